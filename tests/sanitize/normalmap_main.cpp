// normalmap_main.cpp — stand-alone driver of the normal maps' host code for the sanitizers (tests/test_normalmap_ref.py compiles it ALONE, with csrc/rtx_normalmap_host.hpp, under
// -fsanitize=address,undefined and runs it as a child process): the per-triangle tangent records, the height map -> normal map conversion and the green flip, on the inputs of
// a small binary file the test writes.  Its output is compared with the numpy twin (tests/normalmap_ref.py) bit for bit.
// usage: normalmap_main FILE
//   FILE: u32 ntri, ntri x (9 floats corner positions, 6 floats corner pairs); u32 nimg, nimg x (u32 width, u32 height, f64 strength, width * height * 4 bytes)
//   prints per triangle "T" and six hex floats; per image "H" and the converted bytes in hex, "G" and the green-flipped bytes in hex; then "done"
#include <cstdio>
#include <cstring>
#include <vector>
#include "rtx_normalmap_host.hpp"

static bool get(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: normalmap_main FILE");
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the input");
    uint32_t ntri = 0;
    if (!get(f, &ntri, 4) || ntri > 100000u) { fclose(f); return fail("triangle count"); }
    for (uint32_t i = 0; i < ntri; i++) {
        float in[15], out[6];
        if (!get(f, in, sizeof(in))) { fclose(f); return fail("truncated triangle"); }
        rtx::tangent_record(in, in + 9, out);
        printf("T");
        for (int k = 0; k < 6; k++) printf(" %a", (double)out[k]);
        printf("\n");
    }
    uint32_t nimg = 0;
    if (!get(f, &nimg, 4) || nimg > 1000u) { fclose(f); return fail("image count"); }
    for (uint32_t i = 0; i < nimg; i++) {
        uint32_t w = 0, h = 0; double strength = 0.0;
        if (!get(f, &w, 4) || !get(f, &h, 4) || !get(f, &strength, 8) || w < 1 || h < 1 || w > 4096 || h > 4096) { fclose(f); return fail("image header"); }
        std::vector<uint8_t> px((size_t)w * h * 4), nm;
        if (!get(f, px.data(), px.size())) { fclose(f); return fail("truncated image"); }
        rtx::HeightToNormalMap(px.data(), w, h, strength, nm);
        if (nm.size() != px.size()) { fclose(f); return fail("converted size"); }
        printf("H ");
        for (uint8_t b : nm) printf("%02x", b);
        printf("\n");
        rtx::FlipGreen(px.data(), (size_t)w * h);
        printf("G ");
        for (uint8_t b : px) printf("%02x", b);
        printf("\n");
    }
    fclose(f);
    {   std::vector<uint8_t> none;                                       // nothing to flip, nothing to convert from
        rtx::FlipGreen(none.data(), 0);
    }
    printf("done\n");
    return 0;
}
