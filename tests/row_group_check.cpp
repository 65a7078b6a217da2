// Stand-alone host program: csrc/row_group.h's row_cfg over every shape the three kernel families call it with, one line per call
// (tests/test_row_group.py compares the lines with the Python restatement).
#include "row_group.h"

static void put(const char* family, int H, int D, int min_lanes, bool vec4_ok) {
    const wsi::RowCfg c = wsi::row_cfg(H * D, D, min_lanes, vec4_ok);
    printf("%s %d %d %d %d %d %d\n", family, H, D, (int)vec4_ok, c.VEC, c.G, c.NK);
}

int main() {
    for (int ok = 0; ok < 2; ++ok) {
        for (int H = 1; H <= 16; ++H)
            for (int D = 1; H * D <= 4096; ++D) put("gat", H, D, H, ok);
        for (int C = 1; C <= 4096; ++C) put("ra", 1, C, 1, ok);            // (wsi_sddmm_dot calls it the same way)
        for (int D = 1; D <= 1024; ++D) put("gin", 1, D, 1, ok);
    }
    return 0;
}
