// Prints gpak_potrf_plan (gp_ss_ak_amd/csrc/potrf_plan.h) for tests/test_potrf_plan.py.  Built with plain g++ and
// no HIP on the include path: compiling this file is the proof that the header is HIP-free.
//   potrf_plan_driver Np[,Np...] bwd_bw tail_queue bulk_queue side_stream [field=value ...]
// Per size a line "Np <Np>", then one line per panel: J W J2 tail_panel beside_bulk next bulk ticket inv_begin inv_end
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "potrf_plan.h"

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  const int bwd_bw = atoi(argv[2]);
  PotrfCaps caps;
  caps.tail_queue = atoi(argv[3]) != 0;
  caps.bulk_queue = atoi(argv[4]) != 0;
  caps.side_stream = atoi(argv[5]) != 0;
  GpakSchedule s;
  for (int i = 6; i < argc; i++) {
    const char *eq = strchr(argv[i], '=');
    if (!eq) return 2;
    const size_t n = eq - argv[i];
    const int v = atoi(eq + 1);
    auto is = [&](const char *name) { return strlen(name) == n && strncmp(argv[i], name, n) == 0; };
    if (is("nb_outer")) s.nb_outer = v;
    else if (is("nb_wide")) s.nb_wide = v;
    else if (is("nb_wide_rows")) s.nb_wide_rows = v;
    else if (is("nb_xwide")) s.nb_xwide = v;
    else if (is("nb_xwide_rows")) s.nb_xwide_rows = v;
    else if (is("first_narrow")) s.first_narrow = v != 0;
    else if (is("tail_rows")) s.tail_rows = v;
    else if (is("sub_next")) s.sub_next = v != 0;
    else if (is("next_split_rows")) s.next_split_rows = v;
    else if (is("inv512")) s.inv512 = v != 0;
    else if (is("bwd_fused")) s.bwd_fused = v;
    else if (is("lookahead")) s.lookahead = v != 0;
    else if (is("fwd_in_factor")) s.fwd_in_factor = v != 0;
    else return 2;
  }
  for (const char *a = argv[1]; a; a = strchr(a, ',') ? strchr(a, ',') + 1 : nullptr) {
    const int Np = atoi(a);
    printf("Np %d\n", Np);
    for (const PotrfStep &p : gpak_potrf_plan(Np, s, caps, bwd_bw))
      printf("%d %d %d %d %d %d %d %d %d %d\n", p.J, p.W, p.J2, (int)p.tail_panel, (int)p.beside_bulk, (int)p.next,
             (int)p.bulk, p.ticket, p.inv_begin, p.inv_end);
  }
  return 0;
}
