// The marginal tail's geometry as csrc/msm_plan.hpp has it, printed for tests/test_reduction_reference.py: for every window width c given on the command
// line one line "c nb sh0 sh1 sh2 wd0 wd1 wd2", then the buckets marginal_bucket(g, j, v, e) in the order j, v, e.  Host code only.
#include <stdio.h>
#include <stdlib.h>

#include "../../proof_systems_amd/csrc/msm_plan.hpp"

using namespace kh;

int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        const int c = atoi(argv[i]);
        if (c < 2 || c > 17) { fprintf(stderr, "window width %d?\n", c); return 1; }
        const MargGeom g = marginal_geometry((u32)c - 1);
        printf("%d %u %u %u %u %u %u %u\n", c, g.nb, g.sh[0], g.sh[1], g.sh[2], g.wd[0], g.wd[1], g.wd[2]);
        for (u32 j = 0; j < 3; j++)
            for (u32 v = 0; v < (1u << g.wd[j]); v++)
                for (u32 e = 0; e < (g.nb >> g.wd[j]); e++) printf("%u ", marginal_bucket(g, j, v, e));
        printf("\n");
    }
    return 0;
}
