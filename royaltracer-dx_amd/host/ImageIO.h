// ImageIO.h — image writers for the headless display path ("PNG/EXR writers").  The reference
// presents gOutput through a swap chain (Renderer.cpp:554-735) and has no file output; these replace the window.
//   PNG : 8-bit RGBA, zlib "stored" blocks (no compressor dependency), CRC-32 / Adler-32 computed here
//   EXR : OpenEXR 2 single-part scanline file, NO_COMPRESSION, three FLOAT channels B, G, R (linear radiance average)
//   PPM : binary P6
// ... and the READERS of texture maps (map_Kd): no decoder library, so the formats that need none —
//   PPM / PGM : binary P6 / P5, maxval 255 (comments in the header allowed); grey becomes r = g = b
//   TGA       : uncompressed (type 2) and run-length encoded (type 10) true colour, 24 or 32 bits, either vertical origin (descriptor bit 5); no colour map
// Every reader returns top-down RGBA8 (alpha 255 where the file has none); false + err for a missing file, another format or a truncated one.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

bool WritePNG(const std::string& path, const uint8_t* rgba8, uint32_t width, uint32_t height);
bool WritePPM(const std::string& path, const uint8_t* rgba8, uint32_t width, uint32_t height);
// rgba32f: accumulation buffer (xyz = radiance sum, w = sample count) — written as xyz / max(w, 1)
bool WriteEXR(const std::string& path, const float* rgba32f, uint32_t width, uint32_t height);
bool ReadPNM(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& width, uint32_t& height, std::string& err);
bool ReadTGA(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& width, uint32_t& height, std::string& err);
// by content (P5 / P6 magic, else a TGA header that makes sense)
bool ReadImage(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& width, uint32_t& height, std::string& err);
// ... and the file's own channel count: 1 (PGM), 3 (PPM, 24-bit TGA) or 4 (32-bit TGA); untouched on failure
bool ReadImage(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& width, uint32_t& height, uint32_t& channels, std::string& err);
// The alpha byte of an image that serves as an OPACITY map (map_d; include/rtx.h, ALPHA CUT-OUTS): a file with an alpha channel of its own (channels == 4) keeps it, any other
// gets its first (grey / red) channel as alpha.  rgba8: whole RGBA8 pixels (a trailing partial pixel is left alone)
void OpacityAlphaFromChannels(std::vector<uint8_t>& rgba8, uint32_t channels);

// HIGH-DYNAMIC-RANGE images (environment maps), as top-down float RGB (width * height * 3):
//   HDR : Radiance RGBE, FORMAT=32-bit_rle_rgbe, flat or new-style run-length encoded scanlines, the -Y H +X W orientation only; (m, e) -> m * 2^(e - 136), e = 0 -> 0
//   PFM : the colour type "PF", either byte order by the sign of the scale line (its magnitude is not applied), rows bottom-up in the file
bool ReadHDR(const std::string& path, std::vector<float>& rgb32f, uint32_t& width, uint32_t& height, std::string& err);
bool ReadPFM(const std::string& path, std::vector<float>& rgb32f, uint32_t& width, uint32_t& height, std::string& err);
bool ReadHDRImage(const std::string& path, std::vector<float>& rgb32f, uint32_t& width, uint32_t& height, std::string& err);      // by content ("PF" / "#?")
// A latitude-longitude image as the N x N octahedral map of include/rtx.h (rtx_set_environment).  Lat-long convention: column centre phi = 2 pi (x + 0.5) / W, row centre
// theta = pi (y + 0.5) / H from +Y, direction (sin t sin p, cos t, -sin t cos p).  Each octahedral texel is the mean of S x S stratified sub-positions
// ((i + (a + 0.5) / S) / N, (j + (b + 0.5) / S) / N), each looked up NEAREST in the lat-long image (x = floor(p / 2 pi * W), y = floor(t / pi * H), clamped), summed in double
// with b outer and a inner; S = clamp(ceil(W / (2 N)), 2, 16) in double.  out: N * N * 3 floats.  false: a null pointer or a size out of range (N in [1, 2048])
uint32_t LatLongSubSamples(uint32_t W, uint32_t N);
bool LatLongToOctahedral(const float* rgb, uint32_t W, uint32_t H, uint32_t N, float* out);
