// ImageIO.cpp — see ImageIO.h
#include "ImageIO.h"
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
}  // namespace

bool ReadPNM(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& w, uint32_t& h, std::string& err) {
    std::vector<uint8_t> b;
    return read_file(path, b, err) && pnm_from(b, path, rgba8, w, h, err);
}
bool ReadTGA(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& w, uint32_t& h, std::string& err) {
    std::vector<uint8_t> b;
    return read_file(path, b, err) && tga_from(b, path, rgba8, w, h, err);
}
bool ReadImage(const std::string& path, std::vector<uint8_t>& rgba8, uint32_t& w, uint32_t& h, std::string& err) {
    std::vector<uint8_t> b;
    if (!read_file(path, b, err)) return false;
    if (b.size() >= 2 && b[0] == 'P' && (b[1] == '5' || b[1] == '6')) return pnm_from(b, path, rgba8, w, h, err);
    if (!tga_from(b, path, rgba8, w, h, err)) { err = path + ": neither a binary PPM / PGM nor a true-colour TGA (" + err + ")"; return false; }
    return true;
}
