// rtx_map_slots.hpp — the material-map slots of rtx_set_material_map (include/rtx.h) as ONE table: a dense index per slot, and per slot its public value, its name, the
// rule that says which materials it acts on, and the activation group it belongs to.  Everything on the host that is "per slot" is indexed by MapSlot and driven by
// kMapSlots: SceneHost::maps, the device's per-material id table (rtx_ctx::Scene::d_mat_maps), the host layer's Scene::boundMaps.  Host code only; no kernel reads this.
#pragma once
#include <stdint.h>
#include "../../include/rtx.h"

namespace rtx {

enum MapSlot : uint32_t { kMapKd = 0, kMapOpacity, kMapNormal, kMapKs, kMapPr, kMapPm, kMapKe, kMapSlotCount };
// which materials a bound map acts on (include/rtx.h: "an emitter's map has no effect" / EMISSION MAPS)
enum MapRule : uint8_t { kMapAnyMaterial, kMapNotOnEmitter, kMapOnlyOnEmitter };
// what a tiny scene leaves its pre-test records for, and what finalise_scene switches DevScene members by: one bit of MapUse each
enum MapGroup : uint8_t { kGroupKd = 0, kGroupCut, kGroupNrm, kGroupSpc, kGroupEmi };

struct MapSlotDesc { uint32_t api; const char* name; MapRule rule; MapGroup group; };
constexpr MapSlotDesc kMapSlots[kMapSlotCount] = {
    {RTX_MAP_KD,      "RTX_MAP_KD",      kMapAnyMaterial,   kGroupKd},
    {RTX_MAP_OPACITY, "RTX_MAP_OPACITY", kMapNotOnEmitter,  kGroupCut},
    {RTX_MAP_NORMAL,  "RTX_MAP_NORMAL",  kMapNotOnEmitter,  kGroupNrm},
    {RTX_MAP_KS,      "RTX_MAP_KS",      kMapNotOnEmitter,  kGroupSpc},
    {RTX_MAP_PR,      "RTX_MAP_PR",      kMapNotOnEmitter,  kGroupSpc},
    {RTX_MAP_PM,      "RTX_MAP_PM",      kMapNotOnEmitter,  kGroupSpc},
    {RTX_MAP_KE,      "RTX_MAP_KE",      kMapOnlyOnEmitter, kGroupEmi},
};
// the dense index of a public RTX_MAP_* value, or kMapSlotCount for a value that is no slot
inline uint32_t map_slot_of(uint32_t api) { uint32_t s = 0; while (s < kMapSlotCount && kMapSlots[s].api != api) s++; return s; }

// which groups are ACTIVE: some triangle's material has a map of the group bound that acts on it.  SceneHost::map_use() computes it; BuiltScene::map_use is the value AS
// COMMITTED (a tiny scene runs on the general path while any() is set, and the commit that changes the value rebuilds it)
struct MapUse {
    uint8_t groups = 0;
    bool has(MapGroup g) const { return (groups >> g) & 1u; }
    bool kd() const { return has(kGroupKd); }       // DevScene::tri_uv / map_kd are set while any() is
    bool cut() const { return has(kGroupCut); }     // DevScene::tri_cut
    bool nrm() const { return has(kGroupNrm); }     // DevScene::tri_tan / map_nrm
    bool spc() const { return has(kGroupSpc); }     // DevScene::map_ks / map_pr / map_pm (and ess_tab)
    bool emi() const { return has(kGroupEmi); }     // DevScene::map_ke / emi_q
    bool any() const { return groups != 0; }
    bool operator==(const MapUse& o) const { return groups == o.groups; }
    bool operator!=(const MapUse& o) const { return groups != o.groups; }
};

}  // namespace rtx
