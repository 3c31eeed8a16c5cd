// Probe of the diffusion head's routing under the general solver table (csrc/pass_plan.h: vv_head_plan(..., solver_step)) for
// tests/test_solver_family_cpu.py: built for the host only, no HIP call.  One line of input per plan:
//   rows n_steps HF HL MODW p16_ok p16_shift ada_p mod_all head_tail
// and two lines of output: the shipped sampler's plan (has_coef) and the general one, each
//   ada sh_tiles layers seam final_stage solver_step, then vv_head_final of every step
#include <cstdio>
#include "pass_plan.h"

static void show(const VVHeadPlan& p) {
    printf("%d %d %d %d %d %d", p.ada, (int)p.sh_tiles, p.layers, (int)p.seam, p.final_stage, (int)p.solver_step);
    for (int i = 0; i < p.n_steps; ++i) printf(" %d", vv_head_final(p, i));
    printf("\n");
}

int main() {
    int rows, steps, HF, HL, MODW, p16, sh, adap, modall, tail;
    while (scanf("%d %d %d %d %d %d %d %d %d %d", &rows, &steps, &HF, &HL, &MODW, &p16, &sh, &adap, &modall, &tail) == 10) {
        const VVHeadCaps caps{p16 != 0, sh != 0, adap != 0, modall != 0, tail != 0};
        show(vv_head_plan(rows, steps, HF, HL, MODW, caps, true));
        show(vv_head_plan(rows, steps, HF, HL, MODW, caps, true, true));
    }
    return 0;
}
