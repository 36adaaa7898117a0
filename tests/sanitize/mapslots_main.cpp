// mapslots_main.cpp — stand-alone driver of the host scene's map-slot table for the sanitizers (tests/test_host_layer.py compiles it with the host layer and
// tests/sanitize/device_stubs.cpp under -fsanitize=address,undefined and runs it as a child process).  One mesh of four triangles over three materials — a plain one, an
// emitter, one that no triangle uses — and one 2 x 2 texture: every slot is bound to every material in turn, the scene is built, and the committed MapUse, bound_texture and
// the per-triangle cut-out table are compared with the rules of include/rtx.h, written out below by hand.  Then rtx_set_materials' reset and the refused slot values.
// usage: mapslots_main     prints "done"
#include <cstdio>
#include <cstring>
#include <vector>
#include "rtx_scene_host.hpp"

using namespace rtx;

static int fail(const char* what, int slot = -1, int mat = -1) { printf("FAILED: %s (slot %d, material %d)\n", what, slot, mat); return 1; }

enum { PLAIN = 0, EMITTER = 1, UNUSED = 2 };
// include/rtx.h, by hand: the public value of each slot; the group it activates as (kd, cut, nrm, spc, emi); whether it acts on the plain material / on the emitter
struct Expect { uint32_t api; int group; bool on_plain, on_emitter; };
static const Expect kExpect[7] = {
    {0u, 0, true, true},        // RTX_MAP_KD: any material
    {2u, 1, true, false},       // RTX_MAP_OPACITY: an emitter's map has no effect
    {4u, 2, true, false},       // RTX_MAP_NORMAL: likewise
    {6u, 3, true, false},       // RTX_MAP_KS: likewise
    {8u, 3, true, false},       // RTX_MAP_PR: likewise
    {10u, 3, true, false},      // RTX_MAP_PM: likewise
    {12u, 4, false, true},      // RTX_MAP_KE: only on an emitter
};
static bool use_is(const MapUse& u, int group) {      // exactly `group` is active (-1: none)
    const bool g[5] = {u.kd(), u.cut(), u.nrm(), u.spc(), u.emi()};
    for (int k = 0; k < 5; k++) if (g[k] != (k == group)) return false;
    return u.any() == (group >= 0) && (u == MapUse()) == (group < 0);
}
static bool nothing_bound(const SceneHost& H) { for (const std::vector<int32_t>& v : H.maps) if (!v.empty()) return false; return true; }

int main() {
    SceneHost H;
    std::vector<float> mats(3 * 32, 0.0f);
    mats[0] = mats[1] = mats[2] = 0.5f; mats[32 + 9] = 3.0f; mats[64] = 0.25f;      // material 1 emits (Ke.g > 0)
    if (!H.set_materials(mats.data(), 3)) return fail("set_materials");
    const float v[6 * 7] = {0, 0, 0, 0, 0, 1, 0,  1, 0, 0, 0, 0, 1, 0,  1, 1, 0, 0, 0, 1, 0,  0, 1, 0, 0, 0, 1, 0,  2, 0, 1, 0, 0, 1, 0,  2, 1, 1, 0, 0, 1, 0};
    const uint32_t idx[12] = {0, 1, 2, 0, 2, 3, 1, 4, 5, 1, 5, 2};
    const uint32_t mid[12] = {PLAIN, UNUSED, UNUSED, EMITTER, EMITTER, EMITTER, PLAIN, PLAIN, PLAIN, EMITTER, PLAIN, UNUSED};      // the first entry of a triangle counts: plain, emitter, plain, emitter
    const uint32_t tri_mat[4] = {PLAIN, EMITTER, PLAIN, EMITTER};
    uint32_t mesh = 99, inst = 99;
    if (!H.add_mesh(v, 6, idx, 12, mid, &mesh) || mesh != 0) return fail("add_mesh");
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!H.add_instance(0, eye, &inst) || inst != 0) return fail("add_instance");
    const uint32_t texels[4] = {0xFF0000FFu, 0xFF00FF00u, 0xFFFF0000u, 0x80FFFFFFu};
    if (!H.set_texture(0, texels, 2, 2, 0)) return fail("set_texture");
    BuiltScene B;
    if (!H.build(B)) return fail("build without a map");
    if (!use_is(B.map_use, -1) || !use_is(H.map_use(), -1)) return fail("active without a map");

    // ---- a slot value that is odd, or above 12, is refused and changes nothing ----
    H.tex_dirty = false;
    for (uint32_t slot : {1u, 3u, 5u, 7u, 9u, 11u, 13u, 14u, 16u, 0xFFFFFFFFu, 0xFFFFFFFEu})
        if (H.set_material_map(PLAIN, slot, 0)) return fail("an unknown slot was accepted", (int)slot);
    if (H.tex_dirty || !nothing_bound(H) || !use_is(H.map_use(), -1)) return fail("a refused call changed the scene");

    // ---- every slot on every material: the committed MapUse, bound_texture, the per-triangle cut-out table ----
    for (int s = 0; s < 7; s++) for (int m = 0; m < 3; m++) {
        const Expect& e = kExpect[s];
        if (kMapSlots[s].api != e.api || map_slot_of(e.api) != (uint32_t)s) return fail("slot order", s, m);
        if (!H.set_material_map((uint32_t)m, e.api, 0) || !H.tex_dirty) return fail("a valid call was refused", s, m);
        if (!H.build(B)) return fail("build", s, m);
        const bool acts = m == PLAIN ? e.on_plain : m == EMITTER ? e.on_emitter : false;       // (no triangle uses the third material)
        if (!use_is(B.map_use, acts ? e.group : -1) || !(B.map_use == H.map_use())) return fail("MapUse", s, m);
        for (int s2 = 0; s2 < 7; s2++) for (uint32_t m2 = 0; m2 < 5; m2++) {                   // (materials 3 and 4 do not exist)
            const bool emits = m2 == EMITTER;
            const bool want = s2 == s && m2 == (uint32_t)m && (emits ? kExpect[s2].on_emitter : kExpect[s2].on_plain);
            if (H.bound_texture((MapSlot)s2, m2) != (want ? 0 : -1)) return fail("bound_texture", s2, (int)m2);
        }
        if (H.bound_texture(kMapOpacity, 0xFFFFFFFFu) != -1 || H.bound_texture(kMapKe, 0xFFFFFFFFu) != -1 || H.bound_texture(kMapKd, 0xFFFFFFFFu) != -1) return fail("out-of-range material id", s, m);
        std::vector<int32_t> tc; H.fill_tri_cut(tc);
        if (tc.size() != 4) return fail("per-triangle table size", s, m);
        for (int t = 0; t < 4; t++) if (tc[H.insts[0].tri_base + t] != H.bound_texture(kMapOpacity, tri_mat[t])) return fail("fill_tri_cut against bound_texture", s, m);
        if (!H.set_material_map((uint32_t)m, e.api, -1)) return fail("unbind", s, m);
        if (!use_is(H.map_use(), -1)) return fail("active after the unbind", s, m);
    }

    // ---- rtx_set_materials empties every slot, and raises tex_dirty only if something was bound; the energy table stays ----
    std::vector<float> ess(2 * 16, 0.5f);
    if (!H.set_ess_table(ess.data(), 2)) return fail("set_ess_table");
    for (int s = 0; s < 7; s++) if (!H.set_material_map(s == 6 ? EMITTER : PLAIN, kExpect[s].api, 0)) return fail("bind all", s);
    if (!H.build(B)) return fail("build with every slot");
    if (!(B.map_use.kd() && B.map_use.cut() && B.map_use.nrm() && B.map_use.spc() && B.map_use.emi())) return fail("every group");
    H.tex_dirty = false;
    if (!H.set_materials(mats.data(), 3)) return fail("set_materials again");
    if (!H.tex_dirty || !nothing_bound(H) || !use_is(H.map_use(), -1) || H.ess_rows != 2 || H.ess_table.size() != 32) return fail("set_materials with maps bound");
    H.tex_dirty = false;
    if (!H.set_materials(mats.data(), 3)) return fail("set_materials a third time");
    if (H.tex_dirty || !nothing_bound(H)) return fail("set_materials without a map raised tex_dirty");
    if (!H.build(B) || !use_is(B.map_use, -1)) return fail("build after the reset");
    // a slot whose every entry was unbound again counts as nothing bound
    if (!H.set_material_map(PLAIN, 4u, 0) || !H.set_material_map(PLAIN, 4u, -1)) return fail("bind and unbind");
    H.tex_dirty = false;
    if (!H.set_materials(mats.data(), 3) || H.tex_dirty) return fail("set_materials after an unbind raised tex_dirty");
    printf("done\n");
    return 0;
}
