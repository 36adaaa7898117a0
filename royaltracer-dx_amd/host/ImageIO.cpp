// ImageIO.cpp — see ImageIO.h
#include "ImageIO.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
uint32_t crc32_update(uint32_t crc, const uint8_t* p, size_t n) {
    static uint32_t table[256]; static bool init = false;
    if (!init) { for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; table[i] = c; } init = true; }
    for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return crc;
}
void put_be32(std::vector<uint8_t>& v, uint32_t x) { v.push_back((uint8_t)(x >> 24)); v.push_back((uint8_t)(x >> 16)); v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x); }
void put_chunk(std::vector<uint8_t>& out, const char type[4], const std::vector<uint8_t>& data) {
    put_be32(out, (uint32_t)data.size());
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4); out.insert(out.end(), data.begin(), data.end());
    put_be32(out, crc32_update(0xffffffffu, &out[at], 4 + data.size()) ^ 0xffffffffu);
}
bool write_file(const std::string& path, const void* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}
template <class T> void put_le(std::vector<uint8_t>& v, T x) { uint8_t b[sizeof(T)]; memcpy(b, &x, sizeof(T)); v.insert(v.end(), b, b + sizeof(T)); }   // host is little-endian (x86-64)
void put_str(std::vector<uint8_t>& v, const char* s) { v.insert(v.end(), s, s + strlen(s) + 1); }
}  // namespace

bool WritePNG(const std::string& path, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    if (!rgba8 || !w || !h) return false;
    std::vector<uint8_t> raw; raw.reserve((size_t)h * (1 + (size_t)w * 4));
    for (uint32_t y = 0; y < h; y++) { raw.push_back(0); raw.insert(raw.end(), rgba8 + (size_t)y * w * 4, rgba8 + (size_t)(y + 1) * w * 4); }   // filter 0 per scanline
    std::vector<uint8_t> z; z.push_back(0x78); z.push_back(0x01);                       // zlib header, then stored deflate blocks
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < raw.size(); i++) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
    for (size_t at = 0; at < raw.size();) {
        const size_t n = raw.size() - at < 65535 ? raw.size() - at : 65535;
        z.push_back(at + n == raw.size() ? 1 : 0);
        z.push_back((uint8_t)n); z.push_back((uint8_t)(n >> 8)); z.push_back((uint8_t)~n); z.push_back((uint8_t)(~n >> 8));
        z.insert(z.end(), raw.begin() + at, raw.begin() + at + n); at += n;
    }
    put_be32(z, (b << 16) | a);
    std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::vector<uint8_t> ihdr; put_be32(ihdr, w); put_be32(ihdr, h); ihdr.push_back(8); ihdr.push_back(6); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
    put_chunk(out, "IHDR", ihdr); put_chunk(out, "IDAT", z); put_chunk(out, "IEND", {});
    return write_file(path, out.data(), out.size());
}

bool WritePPM(const std::string& path, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    if (!rgba8 || !w || !h) return false;
    char hdr[64]; const int n = snprintf(hdr, sizeof hdr, "P6\n%u %u\n255\n", w, h);
    std::vector<uint8_t> out(hdr, hdr + n); out.reserve(n + (size_t)w * h * 3);
    for (size_t i = 0; i < (size_t)w * h; i++) out.insert(out.end(), rgba8 + i * 4, rgba8 + i * 4 + 3);
    return write_file(path, out.data(), out.size());
}

bool WriteEXR(const std::string& path, const float* acc, uint32_t w, uint32_t h) {
    if (!acc || !w || !h) return false;
    std::vector<uint8_t> o;
    put_le<uint32_t>(o, 20000630u); put_le<uint32_t>(o, 2u);                            // magic, version 2, single-part scanline
    put_str(o, "channels"); put_str(o, "chlist"); put_le<uint32_t>(o, 3 * 18 + 1);
    for (const char* ch : {"B", "G", "R"}) { put_str(o, ch); put_le<uint32_t>(o, 2u /* FLOAT */); put_le<uint32_t>(o, 0u); put_le<uint32_t>(o, 1u); put_le<uint32_t>(o, 1u); }
    o.push_back(0);
    put_str(o, "compression"); put_str(o, "compression"); put_le<uint32_t>(o, 1u); o.push_back(0);
    const int32_t box[4] = {0, 0, (int32_t)w - 1, (int32_t)h - 1};
    for (const char* name : {"dataWindow", "displayWindow"}) { put_str(o, name); put_str(o, "box2i"); put_le<uint32_t>(o, 16u); for (int k = 0; k < 4; k++) put_le<int32_t>(o, box[k]); }
    put_str(o, "lineOrder"); put_str(o, "lineOrder"); put_le<uint32_t>(o, 1u); o.push_back(0);
    put_str(o, "pixelAspectRatio"); put_str(o, "float"); put_le<uint32_t>(o, 4u); put_le<float>(o, 1.0f);
    put_str(o, "screenWindowCenter"); put_str(o, "v2f"); put_le<uint32_t>(o, 8u); put_le<float>(o, 0.0f); put_le<float>(o, 0.0f);
    put_str(o, "screenWindowWidth"); put_str(o, "float"); put_le<uint32_t>(o, 4u); put_le<float>(o, 1.0f);
    o.push_back(0);                                                                     // end of header
    const size_t line_bytes = (size_t)w * 3 * 4, table_at = o.size();
    uint64_t off = table_at + (uint64_t)h * 8;
    for (uint32_t y = 0; y < h; y++) { put_le<uint64_t>(o, off); off += 8 + line_bytes; }
    for (uint32_t y = 0; y < h; y++) {
        put_le<int32_t>(o, (int32_t)y); put_le<uint32_t>(o, (uint32_t)line_bytes);
        for (int c = 2; c >= 0; c--)                                                    // channels in alphabetical order: B, G, R
            for (uint32_t x = 0; x < w; x++) { const float* p = acc + ((size_t)y * w + x) * 4; const float n = p[3] > 1.0f ? p[3] : 1.0f; put_le<float>(o, p[c] / n); }
    }
    return write_file(path, o.data(), o.size());
}

// ------------------------------------------------------------------------------------------------
// readers (texture maps)
// ------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kMaxImageSide = 16384;                  // rtx_set_texture's limit
bool read_file(const std::string& path, std::vector<uint8_t>& out, std::string& err) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open " + path; return false; }
    uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}
bool pnm_from(const std::vector<uint8_t>& b, const std::string& path, std::vector<uint8_t>& rgba, uint32_t& w, uint32_t& h, std::string& err) {
    if (b.size() < 2 || b[0] != 'P' || (b[1] != '5' && b[1] != '6')) { err = path + ": not a binary PPM / PGM (P6 / P5)"; return false; }
    const int ch = b[1] == '6' ? 3 : 1;
    size_t at = 2; uint32_t val[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++) {                          // width, height, maxval: decimal, separated by white space; '#' starts a comment up to the end of the line
        while (at < b.size() && (b[at] == ' ' || b[at] == '\t' || b[at] == '\n' || b[at] == '\r' || b[at] == '#')) { if (b[at] == '#') while (at < b.size() && b[at] != '\n') at++; else at++; }
        bool digit = false;
        while (at < b.size() && b[at] >= '0' && b[at] <= '9' && val[k] < 100000000u) { val[k] = val[k] * 10 + (uint32_t)(b[at] - '0'); at++; digit = true; }
        if (!digit) { err = path + ": bad PNM header"; return false; }
    }
    at++;                                                  // the single white-space byte behind maxval
    if (val[2] != 255) { err = path + ": PNM maxval must be 255"; return false; }
    w = val[0]; h = val[1];
    if (!w || !h || w > kMaxImageSide || h > kMaxImageSide) { err = path + ": image size out of range"; return false; }
    const size_t need = (size_t)w * h * ch;
    if (at > b.size() || b.size() - at < need) { err = path + ": truncated PNM"; return false; }
    rgba.resize((size_t)w * h * 4);
    for (size_t i = 0; i < (size_t)w * h; i++) { const uint8_t* q = &b[at + i * ch]; rgba[i * 4] = q[0]; rgba[i * 4 + 1] = q[ch == 3 ? 1 : 0]; rgba[i * 4 + 2] = q[ch == 3 ? 2 : 0]; rgba[i * 4 + 3] = 255; }
    return true;
}
bool tga_from(const std::vector<uint8_t>& b, const std::string& path, std::vector<uint8_t>& rgba, uint32_t& w, uint32_t& h, std::string& err) {
    if (b.size() < 18) { err = path + ": not a TGA file"; return false; }
    const uint32_t idlen = b[0], cmap = b[1], type = b[2], bpp = b[16], desc = b[17];
    w = b[12] | (b[13] << 8); h = b[14] | (b[15] << 8);
    if (cmap != 0 || (type != 2 && type != 10) || (bpp != 24 && bpp != 32)) { err = path + ": unsupported TGA (true colour, 24 or 32 bits, uncompressed or RLE only)"; return false; }
    if (!w || !h || w > kMaxImageSide || h > kMaxImageSide) { err = path + ": image size out of range"; return false; }
    const size_t cmap_bytes = (size_t)(b[5] | (b[6] << 8)) * ((b[7] + 7u) / 8u);
    size_t at = 18 + (size_t)idlen + cmap_bytes;
    const uint32_t bytes = bpp / 8; const size_t npix = (size_t)w * h;
    rgba.resize(npix * 4);
    const bool top_down = (desc & 0x20u) != 0, right_left = (desc & 0x10u) != 0;
    auto put = [&](size_t i, const uint8_t* q) {           // pixel i in FILE order (b, g, r[, a]) -> its place in the top-down image
        const size_t fy = i / w, fx = i % w, y = top_down ? fy : h - 1 - fy, x = right_left ? w - 1 - fx : fx;
        uint8_t* o = &rgba[(y * w + x) * 4]; o[0] = q[2]; o[1] = q[1]; o[2] = q[0]; o[3] = bytes == 4 ? q[3] : 255;
    };
    if (type == 2) {
        if (at > b.size() || b.size() - at < npix * bytes) { err = path + ": truncated TGA"; return false; }
        for (size_t i = 0; i < npix; i++) put(i, &b[at + i * bytes]);
        return true;
    }
    size_t i = 0;
    while (i < npix) {                                     // packets: header byte, then one pixel repeated (bit 7) or count raw pixels; a packet may cross a row
        if (at >= b.size()) { err = path + ": truncated TGA"; return false; }
        const uint8_t hd = b[at++]; const size_t count = (size_t)(hd & 127u) + 1;
        if (count > npix - i) { err = path + ": TGA packet runs past the image"; return false; }
        if (hd & 128u) {
            if (b.size() - at < bytes) { err = path + ": truncated TGA"; return false; }
            for (size_t k = 0; k < count; k++) put(i + k, &b[at]);
            at += bytes;
        } else {
            if (b.size() - at < count * bytes) { err = path + ": truncated TGA"; return false; }
            for (size_t k = 0; k < count; k++) put(i + k, &b[at + k * bytes]);
            at += count * bytes;
        }
        i += count;
    }
    return true;
}

// ---- high-dynamic-range readers (environment maps): Radiance RGBE and PFM, to top-down float RGB ----
// a header line ending in '\n' starting at `at`; false at the end of the data
bool text_line(const std::vector<uint8_t>& b, size_t& at, std::string& line) {
    line.clear();
    while (at < b.size() && b[at] != '\n') { if (line.size() > 4096) return false; line.push_back((char)b[at++]); }
    if (at >= b.size()) return false;
    at++;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    return true;
}
bool hdr_from(const std::vector<uint8_t>& b, const std::string& path, std::vector<float>& rgb, uint32_t& w, uint32_t& h, std::string& err) {
    size_t at = 0; std::string line;
    if (!text_line(b, at, line) || line.compare(0, 2, "#?") != 0) { err = path + ": not a Radiance picture (no #? signature)"; return false; }
    bool format = false;
    for (;;) {
        if (!text_line(b, at, line)) { err = path + ": truncated Radiance header"; return false; }
        if (line.empty()) break;
        if (line.compare(0, 7, "FORMAT=") == 0) { if (line != "FORMAT=32-bit_rle_rgbe") { err = path + ": Radiance FORMAT other than 32-bit_rle_rgbe"; return false; } format = true; }
    }
    if (!format) { err = path + ": Radiance header without FORMAT=32-bit_rle_rgbe"; return false; }
    if (!text_line(b, at, line)) { err = path + ": truncated Radiance header"; return false; }
    unsigned long hh = 0, ww = 0; char tail = 0;
    if (sscanf(line.c_str(), "-Y %lu +X %lu%c", &hh, &ww, &tail) != 2) { err = path + ": only the -Y H +X W orientation is read"; return false; }
    if (hh < 1 || ww < 1 || hh > 32768 || ww > 32768) { err = path + ": Radiance picture size out of range"; return false; }
    w = (uint32_t)ww; h = (uint32_t)hh;
    rgb.assign((size_t)w * h * 3, 0.0f);
    std::vector<uint8_t> scan((size_t)w * 4);
    for (uint32_t y = 0; y < h; y++) {
        const bool rle = w >= 8 && w < 32768 && b.size() - at >= 4 && b[at] == 2 && b[at + 1] == 2 && (b[at + 2] & 128u) == 0;
        if (rle) {                                            // new-style run-length encoding: the four channels one after the other
            if ((((uint32_t)b[at + 2] << 8) | b[at + 3]) != w) { err = path + ": Radiance scanline length differs from the width"; return false; }
            at += 4;
            for (int ch = 0; ch < 4; ch++) {
                uint32_t x = 0;
                while (x < w) {
                    if (at >= b.size()) { err = path + ": truncated Radiance picture"; return false; }
                    uint32_t count = b[at++];
                    if (count > 128u) {                       // a run
                        count -= 128u;
                        if (count > w - x || at >= b.size()) { err = path + ": corrupt Radiance run"; return false; }
                        const uint8_t v = b[at++];
                        for (uint32_t k = 0; k < count; k++) scan[(size_t)(x + k) * 4 + ch] = v;
                    } else {                                  // literals
                        if (count == 0 || count > w - x || b.size() - at < count) { err = path + ": corrupt Radiance run"; return false; }
                        for (uint32_t k = 0; k < count; k++) scan[(size_t)(x + k) * 4 + ch] = b[at + k];
                        at += count;
                    }
                    x += count;
                }
            }
        } else {                                              // flat: four bytes per pixel
            if (b.size() - at < (size_t)w * 4) { err = path + ": truncated Radiance picture"; return false; }
            memcpy(scan.data(), &b[at], (size_t)w * 4);
            at += (size_t)w * 4;
        }
        for (uint32_t x = 0; x < w; x++) {
            const uint8_t* q = &scan[(size_t)x * 4];
            if (!q[3]) continue;
            const float f = ldexpf(1.0f, (int)q[3] - 136);    // mantissa byte m, exponent byte e: m * 2^(e - 128 - 8)
            float* o = &rgb[((size_t)y * w + x) * 3];
            o[0] = (float)q[0] * f; o[1] = (float)q[1] * f; o[2] = (float)q[2] * f;
        }
    }
    return true;
}
bool pfm_from(const std::vector<uint8_t>& b, const std::string& path, std::vector<float>& rgb, uint32_t& w, uint32_t& h, std::string& err) {
    size_t at = 0; std::string line;
    if (!text_line(b, at, line) || line != "PF") { err = path + ": not a colour PFM (no PF signature)"; return false; }
    unsigned long ww = 0, hh = 0; char tail = 0;
    if (!text_line(b, at, line) || sscanf(line.c_str(), "%lu %lu%c", &ww, &hh, &tail) != 2) { err = path + ": PFM size line"; return false; }
    if (hh < 1 || ww < 1 || hh > 32768 || ww > 32768) { err = path + ": PFM size out of range"; return false; }
    double scale = 0.0;
    if (!text_line(b, at, line) || sscanf(line.c_str(), "%lf%c", &scale, &tail) != 1 || scale == 0.0 || !std::isfinite(scale)) { err = path + ": PFM scale line"; return false; }
    w = (uint32_t)ww; h = (uint32_t)hh;
    const size_t n = (size_t)w * h * 3;
    if (b.size() - at < n * 4) { err = path + ": truncated PFM"; return false; }
    rgb.resize(n);
    const bool little = scale < 0.0;                          // the sign of the scale is the byte order; its magnitude is not applied
    for (uint32_t y = 0; y < h; y++) {                        // rows bottom-up in the file
        const uint8_t* src = &b[at + (size_t)(h - 1u - y) * w * 12];
        for (size_t k = 0; k < (size_t)w * 3; k++) {
            const uint8_t* q = src + k * 4;
            const uint32_t u = little ? ((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24) : ((uint32_t)q[3] | (uint32_t)q[2] << 8 | (uint32_t)q[1] << 16 | (uint32_t)q[0] << 24);
            memcpy(&rgb[(size_t)y * w * 3 + k], &u, 4);
        }
    }
    return true;
}
}  // namespace

bool ReadPNM(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& w, uint32_t& h, std::string& err) {
    std::vector<uint8_t> b;
    return read_file(path, b, err) && pnm_from(b, path, rgba8, w, h, err);
}
bool ReadTGA(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& w, uint32_t& h, std::string& err) {
    std::vector<uint8_t> b;
    return read_file(path, b, err) && tga_from(b, path, rgba8, w, h, err);
}
bool ReadImage(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& w, uint32_t& h, uint32_t& channels, std::string& err) {
    std::vector<uint8_t> b;
    if (!read_file(path, b, err)) return false;
    if (b.size() >= 2 && b[0] == 'P' && (b[1] == '5' || b[1] == '6')) {
        if (!pnm_from(b, path, rgba8, w, h, err)) return false;
        channels = b[1] == '6' ? 3u : 1u;
        return true;
    }
    if (!tga_from(b, path, rgba8, w, h, err)) { err = path + ": neither a binary PPM / PGM nor a true-colour TGA (" + err + ")"; return false; }
    channels = b[16] / 8u;                                  // (tga_from accepted the header: 24 or 32 bits)
    return true;
}
bool ReadImage(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& w, uint32_t& h, std::string& err) {
    uint32_t channels = 0;
    return ReadImage(path, rgba8, w, h, channels, err);
}
void OpacityAlphaFromChannels(std::vector<uint8_t>& rgba8, uint32_t channels) {
    if (channels == 4u) return;
    for (size_t i = 0; i + 3 < rgba8.size(); i += 4) rgba8[i + 3] = rgba8[i];
}

bool ReadHDR(const std::string& path, std::vector<float>& rgb32f, uint32_t& w, uint32_t& h, std::string& err) {
    std::vector<uint8_t> b;
    return read_file(path, b, err) && hdr_from(b, path, rgb32f, w, h, err);
}
bool ReadPFM(const std::string& path, std::vector<float>& rgb32f, uint32_t& w, uint32_t& h, std::string& err) {
    std::vector<uint8_t> b;
    return read_file(path, b, err) && pfm_from(b, path, rgb32f, w, h, err);
}
bool ReadHDRImage(const std::string& path, std::vector<float>& rgb32f, uint32_t& w, uint32_t& h, std::string& err) {
    std::vector<uint8_t> b;
    if (!read_file(path, b, err)) return false;
    if (b.size() >= 2 && b[0] == 'P' && b[1] == 'F') return pfm_from(b, path, rgb32f, w, h, err);
    if (b.size() >= 2 && b[0] == '#' && b[1] == '?') return hdr_from(b, path, rgb32f, w, h, err);
    err = path + ": neither a Radiance .hdr nor a colour .pfm";
    return false;
}

uint32_t LatLongSubSamples(uint32_t W, uint32_t N) {
    const double s = std::ceil((double)W / (2.0 * (double)N));
    return (uint32_t)(s < 2.0 ? 2.0 : s > 16.0 ? 16.0 : s);
}
bool LatLongToOctahedral(const float* rgb, uint32_t W, uint32_t H, uint32_t N, float* out) {
    if (!rgb || !out || W < 1 || H < 1 || N < 1 || N > 2048) return false;
    const double kPi = 3.14159265358979323846;
    const uint32_t S = LatLongSubSamples(W, N);
    for (uint32_t j = 0; j < N; j++) for (uint32_t i = 0; i < N; i++) {
        double sum[3] = {0.0, 0.0, 0.0};
        for (uint32_t sb = 0; sb < S; sb++) for (uint32_t sa = 0; sa < S; sa++) {
            const double u = ((double)i + ((double)sa + 0.5) / (double)S) / (double)N, v = ((double)j + ((double)sb + 0.5) / (double)S) / (double)N;
            double a = 2.0 * u - 1.0, b = 2.0 * v - 1.0;                   // the inverse fold of include/rtx.h, in double
            const double y = (1.0 - std::fabs(a)) - std::fabs(b);
            if (y < 0.0) { const double fa = (1.0 - std::fabs(b)) * (a >= 0.0 ? 1.0 : -1.0), fb = (1.0 - std::fabs(a)) * (b >= 0.0 ? 1.0 : -1.0); a = fa; b = fb; }
            const double inv = 1.0 / std::sqrt((a * a + y * y) + b * b);
            const double dx = a * inv, dy = y * inv, dz = b * inv;
            // (sin t sin p, cos t, -sin t cos p)  ->  t = acos(y), p = atan2(x, -z) in [0, 2 pi)
            const double t = std::acos(dy < -1.0 ? -1.0 : dy > 1.0 ? 1.0 : dy);
            double p = std::atan2(dx, -dz);
            if (p < 0.0) p += 2.0 * kPi;
            long px = (long)std::floor(p / (2.0 * kPi) * (double)W), py = (long)std::floor(t / kPi * (double)H);
            px = px < 0 ? 0 : px > (long)W - 1 ? (long)W - 1 : px; py = py < 0 ? 0 : py > (long)H - 1 ? (long)H - 1 : py;
            const float* q = &rgb[((size_t)py * W + (size_t)px) * 3];
            sum[0] += (double)q[0]; sum[1] += (double)q[1]; sum[2] += (double)q[2];
        }
        float* o = &out[((size_t)j * N + i) * 3];
        for (int k = 0; k < 3; k++) o[k] = (float)(sum[k] / (double)(S * S));
    }
    return true;
}
