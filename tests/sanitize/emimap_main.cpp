// emimap_main.cpp — stand-alone driver of the emission maps' host code (tests/test_emimap_ref.py compiles it with the host scene's sources under -fsanitize=address,undefined
// and runs it as a child process): the scene of a small binary file the test writes goes through rtx::SceneHost — materials, meshes, UVs, instances, textures, RTX_MAP_KE
// slots — and SceneHost::build_lights; its light records, the triangle id and texture of every light and the per-triangle q are printed as hex words and compared with the
// numpy twin (tests/emimap_ref.py) bit for bit.  Then the slot's refusals and rtx_set_materials' reset.
// usage: emimap_main FILE
//   FILE: u32 nmat, nmat x 32 floats; u32 ntex, ntex x (u32 width, height, flags, width * height u32 texels); u32 nmesh, nmesh x (u32 nverts, nverts x 7 floats, u32 nidx,
//         nidx u32 indices, nidx u32 material ids, u32 has_uv, [nidx x 2 floats]); u32 ninst, ninst x (u32 mesh, 16 floats, u32 hidden); nmat i32 emission texture ids
//   prints "A active", "T total-weight bits", per light "L" + 20 words + prim + texture, "Q" + one word per global triangle, "done"
#include <cstdio>
#include <cstring>
#include <vector>
#include "rtx_scene_host.hpp"

static const uint32_t KE = 12u;      // RTX_MAP_KE (11 is not a slot)
static bool get(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }
static uint32_t word(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: emimap_main FILE");
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the input");
    rtx::SceneHost H;
    uint32_t nmat = 0, ntex = 0, nmesh = 0, ninst = 0;
    if (!get(f, &nmat, 4) || nmat == 0 || nmat > 1000u) { fclose(f); return fail("material count"); }
    std::vector<float> mats((size_t)nmat * 32);
    if (!get(f, mats.data(), mats.size() * 4) || !H.set_materials(mats.data(), nmat)) { fclose(f); return fail("materials"); }
    if (!get(f, &ntex, 4) || ntex > 100u) { fclose(f); return fail("texture count"); }
    for (uint32_t t = 0; t < ntex; t++) {
        uint32_t whf[3];
        if (!get(f, whf, 12) || whf[0] == 0 || whf[1] == 0 || whf[0] > 4096u || whf[1] > 4096u) { fclose(f); return fail("texture header"); }
        std::vector<uint32_t> px((size_t)whf[0] * whf[1]);
        if (!get(f, px.data(), px.size() * 4) || !H.set_texture(t, px.data(), whf[0], whf[1], whf[2])) { fclose(f); return fail("texture"); }
    }
    if (!get(f, &nmesh, 4) || nmesh > 100u) { fclose(f); return fail("mesh count"); }
    for (uint32_t m = 0; m < nmesh; m++) {
        uint32_t nv = 0, ni = 0, has_uv = 0, id = 0;
        if (!get(f, &nv, 4) || nv > 100000u) { fclose(f); return fail("vertex count"); }
        std::vector<float> v((size_t)nv * 7);
        if (!get(f, v.data(), v.size() * 4) || !get(f, &ni, 4) || ni > 300000u) { fclose(f); return fail("vertices"); }
        std::vector<uint32_t> idx(ni), mid(ni);
        if (!get(f, idx.data(), (size_t)ni * 4) || !get(f, mid.data(), (size_t)ni * 4) || !get(f, &has_uv, 4)) { fclose(f); return fail("indices"); }
        if (!H.add_mesh(v.data(), nv, idx.data(), ni, mid.data(), &id)) { fclose(f); printf("%s\n", H.err.c_str()); return fail("add_mesh"); }
        if (has_uv) {
            std::vector<float> uv((size_t)ni * 2);
            if (!get(f, uv.data(), uv.size() * 4) || !H.set_mesh_uvs(id, uv.data(), ni)) { fclose(f); return fail("uvs"); }
        }
    }
    if (!get(f, &ninst, 4) || ninst > 1000u) { fclose(f); return fail("instance count"); }
    uint32_t nt = 0;
    for (uint32_t i = 0; i < ninst; i++) {
        uint32_t mesh = 0, hidden = 0, id = 0; float o2w[16]; bool changed = false;
        if (!get(f, &mesh, 4) || !get(f, o2w, 64) || !get(f, &hidden, 4) || !H.add_instance(mesh, o2w, &id)) { fclose(f); return fail("instance"); }
        H.insts[id].tri_base = nt; nt += (uint32_t)(H.meshes[mesh].idx.size() / 3);      // (what a commit's numbering gives)
        if (hidden && !H.set_instance_visible(id, false, &changed)) { fclose(f); return fail("visibility"); }
    }
    std::vector<int32_t> ke(nmat);
    if (!get(f, ke.data(), (size_t)nmat * 4)) { fclose(f); return fail("map ids"); }
    fclose(f);
    // refusals change nothing
    H.tex_dirty = false;
    if (H.set_material_map(0, 11, -1) || H.set_material_map(0, 13, -1) || H.set_material_map(0, 14, -1) || H.set_material_map(nmat, KE, -1) || H.set_material_map(0, KE, (int32_t)ntex) || H.set_material_map(0, KE, -2))
        return fail("an invalid call was accepted");
    if (H.tex_dirty || !H.maps[rtx::kMapKe].empty() || H.any_bound(rtx::kMapKe) || H.map_use().emi()) return fail("a refused call changed the scene");
    for (uint32_t m = 0; m < nmat; m++) if (ke[m] >= 0 && !H.set_material_map(m, KE, ke[m])) return fail("a valid call was refused");
    rtx::BuiltScene B;
    H.build_lights(B);
    const bool emi_active = H.map_use().emi();
    printf("A %d\nT %08x\n", (int)emi_active, word(B.total_weight));
    if (emi_active != !B.emi_q.empty() || (emi_active && (B.emi_q.size() != nt || B.light_emi.size() != B.lights.size() * 2))) return fail("table sizes");
    for (size_t i = 0; i < B.lights.size(); i++) {
        printf("L");
        for (int k = 0; k < 20; k++) printf(" %08x", word(B.lights80[i * 20 + k]));
        printf(" %08x %08x\n", (uint32_t)B.lights[i].prim, (uint32_t)B.lights[i].emi_tex);
    }
    printf("Q");
    for (float q : B.emi_q) printf(" %08x", word(q));
    printf("\n");
    // rtx_set_materials resets the slot: the list of the unmapped scene again
    H.tex_dirty = false;
    if (!H.set_materials(mats.data(), nmat)) return fail("set_materials again");
    if (H.any_bound(rtx::kMapKe) || H.map_use().emi() || !H.maps[rtx::kMapKe].empty()) return fail("set_materials keeps a map");
    H.build_lights(B);
    if (!B.emi_q.empty() || !B.light_emi.empty()) return fail("tables without a map");
    for (const rtx::LightGPU& L : B.lights) if (L.prim != 0u || L.emi_tex != 0) return fail("pad words without a map");
    printf("done\n");
    return 0;
}
