// rtx_texture.hip — diffuse texture maps at the C-ABI of include/rtx.h: per-corner UVs, the texture table, the per-material map slots, and the probe that runs the device's
// sampler for the tests (the per-hit probes of the slots are in rtx_debug.hip).  Host code only: the setters change SceneHost and un-commit the scene; rtx_commit_scene uploads the tables (sync_textures,
// rtx_commit.hip); the device functions are rtx_texture.hpp (rtx_ctx.hpp).
#include "rtx_ctx.hpp"

extern "C" {

// each setter: RTX_ERR_INVALID leaves the scene untouched AND committed; success needs rtx_commit_scene again
int rtx_set_mesh_uvs(rtx_ctx* c, uint32_t mesh, const float* uv2, uint32_t nidx) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->host.set_mesh_uvs(mesh, uv2, nidx)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    c->committed = false; return RTX_OK;
}
int rtx_set_texture(rtx_ctx* c, uint32_t tex, const void* rgba8, uint32_t width, uint32_t height, uint32_t flags) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->host.set_texture(tex, rgba8, width, height, flags)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    c->committed = false; return RTX_OK;
}
int rtx_set_material_map(rtx_ctx* c, uint32_t material, uint32_t slot, int32_t tex) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->host.set_material_map(material, slot, tex)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    c->committed = false; return RTX_OK;
}
int rtx_set_ess_table(rtx_ctx* c, const float* table, uint32_t rows) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->host.set_ess_table(table, rows)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    c->committed = false; return RTX_OK;
}

int rtx_debug_texture_sample(rtx_ctx* c, uint32_t tex, const float* uv2, uint32_t n, float* out4) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (tex >= c->dsc.ntex) { c->err = "texture_sample: unknown texture"; return RTX_ERR_INVALID; }
    if (!n) return RTX_OK;
    if (!uv2 || !out4) { c->err = "texture_sample: null array"; return RTX_ERR_INVALID; }
    DevBuf d_uv, d_out;
    HIPCHK(c, d_uv.ensure((size_t)n * 8)); HIPCHK(c, d_out.ensure((size_t)n * 16));
    TO_DEVICE(c, d_uv.p, uv2, (size_t)n * 8);
    launch_dbg_tex_sample(c->stream, c->dsc, tex, (const float*)d_uv.p, n, (F4*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out4, d_out.p, (size_t)n * 16);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

}  // extern "C"
