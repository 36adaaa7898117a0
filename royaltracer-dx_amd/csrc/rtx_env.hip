// rtx_env.hip — environment lighting at the C-ABI of include/rtx.h: rtx_set_environment and the three probes that run the device's sampler and lookup for the tests.
// Host code only: the setter changes SceneHost and un-commits the scene; rtx_commit_scene builds and uploads the tables (sync_environment, rtx_commit.hip; the builder:
// rtx_env_host.cpp); the device functions are rtx_env.hpp.
#include "rtx_ctx.hpp"

namespace {
// the scene as the probes see it: the tables of the bound map, also of a black one (which the frame kernels never read)
int env_scene(rtx_ctx* c, const char* what, DevScene& sc) {
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (!c->dsc.env_n) { c->err = std::string(what) + ": no environment bound"; return RTX_ERR_STATE; }
    sc = c->dsc;
    sc.env_tex = (const F4*)c->scene.d_env_tex.p; sc.env_marg = (const float*)c->scene.d_env_marg.p; sc.env_cond = (const float*)c->scene.d_env_cond.p;
    return RTX_OK;
}
}  // namespace

extern "C" {

// RTX_ERR_INVALID leaves the scene untouched AND committed; success needs rtx_commit_scene again
int rtx_set_environment(rtx_ctx* c, const float* rgb32f, uint32_t n, const float* env_to_world, float scale, uint32_t flags) {
    if (!c) return RTX_ERR_INVALID;
    if (!rgb32f) {                                            // clear
        if (c->host.env.n) { c->host.env = EnvHost{}; c->host.env_dirty = true; c->committed = false; }
        return RTX_OK;
    }
    if (!env_set(c->host.env, rgb32f, n, env_to_world, scale, flags, c->err)) return RTX_ERR_INVALID;
    c->host.env_dirty = true; c->committed = false;
    return RTX_OK;
}

int rtx_debug_env_tables(rtx_ctx* c, float* texels4, float* marginal, float* conditional) {
    BIND(c);
    DevScene sc; int r = env_scene(c, "env_tables", sc); if (r) return r;
    const size_t n = sc.env_n;
    if (texels4) TO_HOST(c, texels4, sc.env_tex, n * n * 16);
    if (marginal) TO_HOST(c, marginal, sc.env_marg, n * 4);
    if (conditional) TO_HOST(c, conditional, sc.env_cond, n * n * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
int rtx_debug_env_sample(rtx_ctx* c, const uint32_t* seeds2, uint32_t n, float* out12) {
    BIND(c);
    DevScene sc; int r = env_scene(c, "env_sample", sc); if (r) return r;
    if (!(c->scene.env_total > 0.0)) { c->err = "env_sample: the environment has no weight, so nothing samples it"; return RTX_ERR_STATE; }
    if (!n) return RTX_OK;
    if (!seeds2 || !out12) { c->err = "env_sample: null array"; return RTX_ERR_INVALID; }
    DevBuf d_in, d_out;
    HIPCHK(c, d_in.ensure((size_t)n * 8)); HIPCHK(c, d_out.ensure((size_t)n * 48));
    TO_DEVICE(c, d_in.p, seeds2, (size_t)n * 8);
    launch_dbg_env_sample(c->stream, sc, (const uint32_t*)d_in.p, n, (F4*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out12, d_out.p, (size_t)n * 48);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
int rtx_debug_env_eval(rtx_ctx* c, const float* dirs3, uint32_t n, float* out8) {
    BIND(c);
    DevScene sc; int r = env_scene(c, "env_eval", sc); if (r) return r;
    if (!n) return RTX_OK;
    if (!dirs3 || !out8) { c->err = "env_eval: null array"; return RTX_ERR_INVALID; }
    DevBuf d_in, d_out;
    HIPCHK(c, d_in.ensure((size_t)n * 12)); HIPCHK(c, d_out.ensure((size_t)n * 32));
    TO_DEVICE(c, d_in.p, dirs3, (size_t)n * 12);
    launch_dbg_env_eval(c->stream, sc, (const float*)d_in.p, n, (F4*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out8, d_out.p, (size_t)n * 32);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

}  // extern "C"
