// Prints gpak_potrf_caps and gpak_potrf_block_co (gp_ss_ak_amd/csrc/potrf_plan.h) for tests/test_potrf_caps.py.  Built with
// plain g++ and no HIP on the include path, like potrf_plan_driver.cpp.
//   potrf_caps_driver caps Np[,Np...] bwd_bw tail_queue_max_np     (tail_queue_max_np < 0: the struct's default)
//     first a line "default <tail_queue_max_np of GpakSchedule>", then per size and per combination of streams a line
//     "Np <Np> <have_tail> <have_bulk> <have_side> <caps.tail_queue> <caps.bulk_queue> <caps.side_stream>" and the plan
//     made from those caps, one line per panel as potrf_plan_driver prints it
//   potrf_caps_driver co cu_count surplus_pct
//     per potrf_co in 0, 1, 2, beside_bulk in 0, 1 and mt (tile rows of the bulk update beside the panel) in 0..64:
//     "<potrf_co> <beside_bulk> <mt> <workgroups> <co>"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "potrf_plan.h"

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "caps")) {
    const int bwd_bw = atoi(argv[3]);
    GpakSchedule s;
    printf("default %d\n", s.tail_queue_max_np);
    if (atoi(argv[4]) >= 0) s.tail_queue_max_np = atoi(argv[4]);
    for (const char *a = argv[2]; a; a = strchr(a, ',') ? strchr(a, ',') + 1 : nullptr) {
      const int Np = atoi(a);
      for (int m = 0; m < 8; m++) {
        const bool ht = m & 1, hb = m & 2, hs = m & 4;
        const PotrfCaps caps = gpak_potrf_caps(Np, s, ht, hb, hs);
        printf("Np %d %d %d %d %d %d %d\n", Np, (int)ht, (int)hb, (int)hs, (int)caps.tail_queue, (int)caps.bulk_queue,
               (int)caps.side_stream);
        for (const PotrfStep &p : gpak_potrf_plan(Np, s, caps, bwd_bw))
          printf("%d %d %d %d %d %d %d %d %d %d\n", p.J, p.W, p.J2, (int)p.tail_panel, (int)p.beside_bulk, (int)p.next,
                 (int)p.bulk, p.ticket, p.inv_begin, p.inv_end);
      }
    }
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "co")) {
    const int cu = atoi(argv[2]), surplus = atoi(argv[3]);
    for (int co = 0; co <= 2; co++)
      for (int beside = 0; beside <= 1; beside++)
        for (int mt = 0; mt <= 64; mt++) {
          PotrfStep st;
          st.beside_bulk = beside != 0;
          const long wg = gpak_bulk_workgroups(mt, surplus);
          printf("%d %d %d %ld %d\n", co, beside, mt, wg, (int)gpak_potrf_block_co(st, co, wg, cu));
        }
    return 0;
  }
  return 2;
}
