// Replays events through CtxState (gp_ss_ak_amd/csrc/ctx_state.h) for tests/test_ctx_state.py.  Built with plain g++ and
// no HIP on the include path: compiling this file is the proof that the header is HIP-free.
// Reads one event per line from the standard input -- the name of a member of CtxState, with its arguments where it has
// some ("factorisation_succeeded <fwd_in_factor> <inv512> <bwd_fused>", "factorisation_failed <col>", "set_memoise <0|1>");
// "reset" starts a fresh context.  After each line prints the whole state:
//   points rung z backsolve image failed_col factorisations
#include <cstdio>
#include <cstring>

#include "ctx_state.h"

int main() {
  CtxState s;
  char line[256], ev[64];
  while (fgets(line, sizeof(line), stdin)) {
    int a = 0, b = 0, c = 0;
    if (sscanf(line, "%63s %d %d %d", ev, &a, &b, &c) < 1) continue;
    auto is = [&](const char *name) { return strcmp(ev, name) == 0; };
    if (is("reset")) s = CtxState();
    else if (is("set_memoise")) s.set_memoise(a != 0);
    else if (is("new_training_set")) s.new_training_set();
    else if (is("new_kernel")) s.new_kernel();
    else if (is("same_kernel")) s.same_kernel();
    else if (is("points_built")) s.points_built();
    else if (is("matrix_overwritten")) s.matrix_overwritten();
    else if (is("factorisation_started")) s.factorisation_started();
    else if (is("factorisation_succeeded")) s.factorisation_succeeded(a != 0, b != 0, c);
    else if (is("factorisation_failed")) s.factorisation_failed(a);
    else if (is("factor_imported")) s.factor_imported();
    else if (is("work_vectors_overwritten")) s.work_vectors_overwritten();
    else if (is("alpha_built")) s.alpha_built();
    else if (is("nlz_built")) s.nlz_built();
    else if (is("image_built")) s.image_built();
    else { fprintf(stderr, "unknown event: %s\n", ev); return 2; }
    printf("%d %d %d %d %d %d %d\n", (int)s.points, (int)s.rung, (int)s.z, (int)s.backsolve, (int)s.image, s.failed_col,
           s.factorisations);
  }
  return 0;
}
