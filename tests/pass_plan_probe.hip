// Probe of the pass routing (csrc/pass_plan.h: vv_lm_pass_plan, vv_head_plan) for tests/test_pass_plan_cpu.py: built for the host
// alone (no device code, no GPU).  Reads one case per line from stdin, the first word names the plan:
//   lm   ws_rows attn_splits Hkv tile3_ok attn2_ok p16_ok n_rows (cache pos) x n_rows
//          ->  rc fused contiguous [route attn attn_S attn_groups zero_v_tail key_mode key_split kv_positions]   (rc 0 only)
//   head rows n_steps HF HL MODW p16_ok p16_shift ada_p mod_all head_tail has_coef
//          ->  ada sh_tiles layers solver_step, then the final stage of every step
#include <cstdio>
#include <cstring>
#include <vector>
#include "pass_plan.h"

int main() {
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        if (!strcmp(kind, "lm")) {
            int ws, splits, Hkv, t3, a2, p16, n;
            if (scanf("%d %d %d %d %d %d %d", &ws, &splits, &Hkv, &t3, &a2, &p16, &n) != 7 || n < 1) return 1;
            std::vector<VVRow> rows(n);
            for (auto& r : rows) if (scanf("%d %d", &r.cache, &r.pos) != 2) return 1;
            VVLmPlan p = {};
            const int rc = vv_lm_pass_plan(rows.data(), n, VVLmCaps{ws, splits, Hkv, t3 != 0, a2 != 0, p16 != 0}, &p);
            if (rc) printf("%d %d %d\n", rc, (int)p.fused, (int)p.contiguous);
            else printf("%d %d %d %d %d %d %d %d %d %d %lld\n", rc, (int)p.fused, (int)p.contiguous, p.route, p.attn, p.attn_S, p.attn_groups,
                        (int)p.zero_v_tail, p.key_mode, p.key_split, (long long)p.kv_positions);
        } else if (!strcmp(kind, "head")) {
            int rows, steps, HF, HL, MODW, p16, sh, adap, modall, tail, coef;
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d", &rows, &steps, &HF, &HL, &MODW, &p16, &sh, &adap, &modall, &tail, &coef) != 11) return 1;
            const VVHeadPlan p = vv_head_plan(rows, steps, HF, HL, MODW, VVHeadCaps{p16 != 0, sh != 0, adap != 0, modall != 0, tail != 0}, coef != 0);
            printf("%d %d %d %d", p.ada, (int)p.sh_tiles, p.layers, (int)p.solver_step);
            for (int i = 0; i < steps; ++i) printf(" %d", vv_head_final(p, i));
            printf("\n");
        } else return 1;
    }
    return 0;
}
