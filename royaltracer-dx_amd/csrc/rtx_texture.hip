// rtx_texture.hip — diffuse texture maps at the C-ABI of include/rtx.h: per-corner UVs, the texture table, the per-material map slot, and the two probes that run the device's
// sampler and per-hit albedo for the tests.  Host code only: the setters change SceneHost and un-commit the scene; rtx_commit_scene uploads the tables (sync_textures,
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
// rays8 is taken for symmetry with rtx_debug_surface; the albedo depends on the hit record alone (triangle id and barycentrics)
int rtx_debug_albedo(rtx_ctx* c, const float* rays8, const float* hits4, uint32_t n, float* out4) {
    BIND(c);
    (void)rays8;
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (!n) return RTX_OK;
    if (!hits4 || !out4) { c->err = "albedo: null array"; return RTX_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++) {                       // a triangle id the scene does not have would index past the per-triangle tables
        uint32_t prim; memcpy(&prim, &hits4[(size_t)i * 4 + 3], 4);
        if (prim != kMissPrim && prim >= c->stats.triangles) { c->err = "albedo: triangle id out of range"; return RTX_ERR_INVALID; }
    }
    DevBuf d_hits, d_out;
    HIPCHK(c, d_hits.ensure((size_t)n * 16)); HIPCHK(c, d_out.ensure((size_t)n * 16));
    TO_DEVICE(c, d_hits.p, hits4, (size_t)n * 16);
    launch_dbg_albedo(c->stream, c->dsc, (const F4*)d_hits.p, n, (F4*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out4, d_out.p, (size_t)n * 16);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

// hits4 as rtx_debug_trace_closest writes them -> (alpha as the traversal computes it, opacity texture id as uint bits): cut_alpha of rtx_cutout.hpp, the function cut_accept compares
int rtx_debug_opacity(rtx_ctx* c, const float* hits4, uint32_t n, float* out2) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (!n) return RTX_OK;
    if (!hits4 || !out2) { c->err = "opacity: null array"; return RTX_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++) {                       // a triangle id the scene does not have would index past the per-triangle tables
        uint32_t prim; memcpy(&prim, &hits4[(size_t)i * 4 + 3], 4);
        if (prim != kMissPrim && prim >= c->stats.triangles) { c->err = "opacity: triangle id out of range"; return RTX_ERR_INVALID; }
    }
    DevBuf d_hits, d_out;
    HIPCHK(c, d_hits.ensure((size_t)n * 16)); HIPCHK(c, d_out.ensure((size_t)n * 8));
    TO_DEVICE(c, d_hits.p, hits4, (size_t)n * 16);
    launch_dbg_opacity(c->stream, c->dsc, (const F4*)d_hits.p, n, (float*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out2, d_out.p, (size_t)n * 8);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

}  // extern "C"
