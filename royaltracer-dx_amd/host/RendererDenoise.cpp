// RendererDenoise.cpp — Renderer::Denoise and the reads of the denoised image (Renderer.h).  Its own translation unit: the rest of the facade links against the entry points
// the device API has had since the host layer was written, and is built that way with a stubbed device (the sanitizer runs of the host layer); this part needs rtx_denoise.
#include <stdexcept>
#include "../../include/rtx_host.h"
#include "Renderer.h"

rtx_denoise_result Renderer::Denoise(const rtx_denoise_params* params) {
    if (m_mode == Mode::ReSTIR) throw std::logic_error("Renderer::Denoise: the ReSTIR frame has its own reuse passes; the filter's guides assume the path tracer's accumulation");
    rtx_denoise_result res{};
    Check(rtx_denoise(m_ctx, m_width, m_height, params, &res), "rtx_denoise");
    return res;
}
rtx_denoise_result Renderer::DenoiseVariance(const rtx_denoise_var_params* params) {
    if (m_mode == Mode::ReSTIR) throw std::logic_error("Renderer::DenoiseVariance: the ReSTIR frame has its own reuse passes; the filter's guides assume the path tracer's accumulation");
    rtx_denoise_result res{};
    Check(rtx_denoise_variance(m_ctx, m_width, m_height, params, &res), "rtx_denoise_variance");
    return res;
}
std::vector<float> Renderer::ReadDenoised() {
    std::vector<float> v((size_t)m_width * m_height * 4);
    Check(rtx_read_denoised(m_ctx, v.data(), v.size() * 4), "rtx_read_denoised");
    return v;
}
std::vector<uint8_t> Renderer::ReadDenoisedOutput() {
    std::vector<uint8_t> v((size_t)m_width * m_height * 4);
    Check(rtx_read_denoised_srgb8(m_ctx, v.data(), v.size()), "rtx_read_denoised_srgb8");
    return v;
}

// the C wrapper of Renderer::DenoiseVariance (include/rtx_host.h).  Here and not in rtx_host_c.cpp for the reason above: that file links without the denoiser's entry points
extern "C" int rtxh_renderer_denoise_variance(rtxh_renderer* r, const rtx_denoise_var_params* params, rtx_denoise_result* out) {
    if (!r || !r->r->Context()) return RTX_ERR_STATE;
    try { const rtx_denoise_result res = r->r->DenoiseVariance(params); if (out) *out = res; return RTX_OK; }
    catch (const std::logic_error&) { return RTX_ERR_STATE; }
    catch (const std::exception&) { return RTX_ERR_INVALID; }
}
