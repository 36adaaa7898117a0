// specmap_main.cpp — stand-alone driver of the specular maps' host code for the sanitizers (tests/test_specmap_ref.py compiles it ALONE, with csrc/rtx_specmap_host.hpp, under
// -fsanitize=address,undefined and runs it as a child process): the energy table's validation, the row arithmetic of its look-up and the loader's zero-scalar rule, on the
// inputs of a small binary file the test writes.  Its output is compared with the numpy twin (tests/specmap_ref.py) bit for bit.
// usage: specmap_main FILE
//   FILE: u32 ntab, ntab x (u32 rows, u32 nvalues, nvalues floats; u32 npr, npr floats)      (nvalues = rows * 16 for a well-formed table; rows outside [2, 256] are only validated)
//         u32 nrec, nrec x (5 floats: Ks.xyz, Pr, Pm)
//   prints per table "V ok" or "V <message>", and for a valid one per roughness "R r0 r1 wr" and "B" with the 16 blended values as hex floats; per record "Z" with the
//   five values after the rule and the three change flags; then "done"
#include <cstdio>
#include <cstring>
#include <vector>
#include "rtx_specmap_host.hpp"

static bool get(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }

int main(int argc, char** argv) {
    if (argc != 2) return fail("usage: specmap_main FILE");
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the input");
    uint32_t ntab = 0;
    if (!get(f, &ntab, 4) || ntab > 1000u) { fclose(f); return fail("table count"); }
    for (uint32_t i = 0; i < ntab; i++) {
        uint32_t rows = 0, nval = 0, npr = 0;
        if (!get(f, &rows, 4) || !get(f, &nval, 4) || nval > 65536u) { fclose(f); return fail("table header"); }
        std::vector<float> tab(nval);
        if (!get(f, tab.data(), (size_t)nval * 4)) { fclose(f); return fail("truncated table"); }
        if (!get(f, &npr, 4) || npr > 100000u) { fclose(f); return fail("roughness count"); }
        std::vector<float> pr(npr);
        if (!get(f, pr.data(), (size_t)npr * 4)) { fclose(f); return fail("truncated roughness list"); }
        // (the validation reads rows * 16 values: only a table that holds them is handed over with its row count)
        const bool sized = (size_t)rows * rtx::kEssCols == nval;
        const char* e = sized ? rtx::ess_table_error(nval ? tab.data() : nullptr, rows) : "size";
        printf("V %s\n", e ? e : "ok");
        if (e || !rows) continue;
        for (float p : pr) {
            const rtx::EssRows R = rtx::ess_rows_of(p, rows);
            printf("R %u %u %a\n", R.r0, R.r1, (double)R.wr);
            float out[16];
            rtx::ess_blend_row(tab.data(), rows, p, out);
            printf("B");
            for (int k = 0; k < 16; k++) printf(" %a", (double)out[k]);
            printf("\n");
        }
    }
    uint32_t nrec = 0;
    if (!get(f, &nrec, 4) || nrec > 100000u) { fclose(f); return fail("record count"); }
    for (uint32_t i = 0; i < nrec; i++) {
        float r[5];
        if (!get(f, r, sizeof(r))) { fclose(f); return fail("truncated record"); }
        const bool ck = rtx::spec_unit_colour(r), cr = rtx::spec_unit_scalar(r + 3), cm = rtx::spec_unit_scalar(r + 4);
        printf("Z");
        for (int k = 0; k < 5; k++) printf(" %a", (double)r[k]);
        printf(" %d %d %d\n", (int)ck, (int)cr, (int)cm);
    }
    fclose(f);
    printf("done\n");
    return 0;
}
