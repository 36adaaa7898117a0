// cutout_main.cpp — stand-alone driver of the cut-outs' host code for the sanitizers (tests/test_cutout_ref.py compiles it with the host layer and tests/sanitize/device_stubs.cpp
// under -fsanitize=address,undefined and runs it as a child process): the image reader's channel count and the alpha conversion on every file named on the command line — the
// good ones and the truncated / corrupt ones alike — and the host scene's opacity-map table through rtx_set_materials, out-of-range ids and the per-triangle table.
// usage: cutout_main FILE...     prints one line per file ("ok W H channels alpha-sum" / "refused: why") and "done"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "rtx_scene_host.hpp"
#include "ImageIO.h"

static const uint32_t OPA = 2u;      // RTX_MAP_OPACITY (1 is not a slot)
static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }

int main(int argc, char** argv) {
    // ---- the reader's channel count and the alpha rule ----
    for (int i = 1; i < argc; i++) {
        std::vector<uint8_t> px; uint32_t w = 0, h = 0, ch = 77; std::string err;
        if (!ReadImage(argv[i], px, w, h, ch, err)) { if (ch != 77) return fail("a refused file changed the channel count"); printf("refused: %s\n", err.c_str()); continue; }
        if (px.size() != (size_t)w * h * 4) return fail("reader returned another size than it reports");
        if (ch != 1 && ch != 3 && ch != 4) return fail("channel count");
        std::vector<uint8_t> plain; uint32_t w2 = 0, h2 = 0;
        if (!ReadImage(argv[i], plain, w2, h2, err) || plain != px || w2 != w || h2 != h) return fail("the two overloads disagree");
        const std::vector<uint8_t> before = px;
        OpacityAlphaFromChannels(px, ch);
        unsigned long long sum = 0;
        for (size_t k = 0; k < px.size(); k += 4) {
            if (px[k] != before[k] || px[k + 1] != before[k + 1] || px[k + 2] != before[k + 2]) return fail("the conversion changed a colour byte");
            if (px[k + 3] != (ch == 4 ? before[k + 3] : before[k])) return fail("alpha byte");
            sum += px[k + 3];
        }
        printf("ok %u %u %u %llu\n", w, h, ch, sum);
    }
    {   std::vector<uint8_t> none, odd = {1, 2, 3, 4, 5, 6, 7};          // empty and a trailing partial pixel
        OpacityAlphaFromChannels(none, 1); OpacityAlphaFromChannels(odd, 3);
        if (!none.empty() || odd != std::vector<uint8_t>({1, 2, 3, 1, 5, 6, 7})) return fail("partial pixel");
    }
    // ---- the opacity-map table of the host scene ----
    rtx::SceneHost H;
    std::vector<float> mats(3 * 32, 0.0f);
    mats[0] = mats[1] = mats[2] = 0.5f; mats[32] = 0.25f; mats[64 + 9] = 3.0f;      // material 2 emits (Ke.g > 0)
    if (!H.set_materials(mats.data(), 3)) return fail("set_materials");
    const float v[4 * 7] = {0, 0, 0, 0, 0, 1, 0,  1, 0, 0, 0, 0, 1, 0,  1, 1, 0, 0, 0, 1, 0,  0, 1, 0, 0, 0, 1, 0};
    const uint32_t idx[9] = {0, 1, 2, 0, 2, 3, 0, 1, 3}, mid[9] = {0, 2, 2, 1, 0, 0, 2, 1, 1};      // the triangles' materials: 0, 1, 2 (the first entry counts)
    uint32_t mesh = 99, inst = 99;
    if (!H.add_mesh(v, 4, idx, 9, mid, &mesh) || mesh != 0) return fail("add_mesh");
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!H.add_instance(0, eye, &inst) || !H.add_instance(0, eye, &inst)) return fail("add_instance");
    H.insts[1].tri_base = 3;                                                       // (what a commit's numbering gives two instances of a 3-triangle mesh)
    const uint32_t texel = 0x80FFFFFFu;
    if (!H.set_texture(0, &texel, 1, 1, 0) || !H.set_texture(1, &texel, 1, 1, 1)) return fail("set_texture");
    if (H.map_use().cut() || H.any_bound(rtx::kMapOpacity)) return fail("active without a map");
    // refusals change nothing
    H.tex_dirty = false;
    if (H.set_material_map(3, OPA, 0) || H.set_material_map(0, 1, 0) || H.set_material_map(0, 3, 0) || H.set_material_map(0, OPA, 2) || H.set_material_map(0, OPA, -2) || H.set_material_map(0xFFFFFFFFu, OPA, 0)) return fail("an invalid call was accepted");
    if (H.tex_dirty || !H.maps[rtx::kMapOpacity].empty() || !H.maps[rtx::kMapKd].empty()) return fail("a refused call changed the scene");
    // an emitter's map has no effect
    if (!H.set_material_map(2, OPA, 0)) return fail("a valid call was refused");
    if (!H.any_bound(rtx::kMapOpacity) || H.map_use().cut() || !H.tex_dirty) return fail("an emitter's map");
    if (!H.set_material_map(1, OPA, 1) || !H.set_material_map(1, 0, 1)) return fail("both slots, one texture");
    if (!H.map_use().cut() || !H.map_use().kd() || H.maps[rtx::kMapKd][1] != 1 || H.maps[rtx::kMapOpacity][1] != 1) return fail("slots");
    std::vector<int32_t> tc; H.fill_tri_cut(tc);
    if (tc != std::vector<int32_t>({-1, 1, -1, -1, 1, -1})) return fail("per-triangle table");
    if (H.bound_texture(rtx::kMapOpacity, 7) != -1 || H.bound_texture(rtx::kMapOpacity, 0xFFFFFFFFu) != -1) return fail("out-of-range material id");
    std::vector<float> uv; H.fill_tri_uv(uv);
    if (uv.size() != 36) return fail("uv table");
    // unbinding, and rtx_set_materials: every map back to -1
    if (!H.set_material_map(1, OPA, -1) || H.map_use().cut() || !H.map_use().kd()) return fail("unbind");
    if (!H.set_material_map(0, OPA, 0) || !H.map_use().cut()) return fail("rebind");
    H.tex_dirty = false;
    if (!H.set_materials(mats.data(), 2)) return fail("set_materials again");
    bool any_map = false; for (uint32_t s = 0; s < rtx::kMapSlotCount; s++) any_map = any_map || H.any_bound((rtx::MapSlot)s);
    if (!H.tex_dirty || any_map || H.map_use().cut() || H.map_use().kd()) return fail("set_materials keeps a map");
    H.fill_tri_cut(tc);                                                            // material ids 2 are now out of range: no cut-out, no read past the table
    for (int32_t t : tc) if (t != -1) return fail("table after set_materials");
    if (H.set_material_map(2, OPA, 0)) return fail("a material beyond the new table");
    printf("done\n");
    return 0;
}
