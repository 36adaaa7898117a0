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
