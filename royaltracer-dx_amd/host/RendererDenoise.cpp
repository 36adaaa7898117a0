// RendererDenoise.cpp — Renderer::Denoise and the reads of the denoised image (Renderer.h).  Its own translation unit: the rest of the facade links against the entry points
// the device API has had since the host layer was written, and is built that way with a stubbed device (the sanitizer runs of the host layer); this part needs rtx_denoise.
#include <stdexcept>
#include "Renderer.h"

rtx_denoise_result Renderer::Denoise(const rtx_denoise_params* params) {
    if (m_mode == Mode::ReSTIR) throw std::logic_error("Renderer::Denoise: the ReSTIR frame has its own reuse passes; the filter's guides assume the path tracer's accumulation");
    rtx_denoise_result res{};
    Check(rtx_denoise(m_ctx, m_width, m_height, params, &res), "rtx_denoise");
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
