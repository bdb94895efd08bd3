// Replays GEMM calls through the planner (csrc/gemm_plan.h) on the host: one call per input line, one line out with
// the launch sequence the plan stands for, in the notation of tests/golden/gemm_plan.json (tests/test_gemm_plan.py).
//   gemm layout epi M N K lda ldb splits dbias sched | wgrad M N K lda ldb splits sched |
//   wgrad_kt M N K splits sched | wgrad_grouped count M0 N0 .. K splits sched          (argv[1]: the CU count)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gemm_plan.h"

using namespace gpt2mi;

static void print_plan(const GemmPlan& p) {
  if (p.family == GemmFamily::Refused) {
    puts("refused");
    return;
  }
  const char* fam = p.family == GemmFamily::TwoStage256 ? "g256" : p.family == GemmFamily::Tile128 ? "g128" : "pp";
  printf("%s %d%d%d%d%d%d%d%d %d %d %d", fam, (int)p.a_t, (int)p.b_t, p.epi, p.map,
         (int)(p.family == GemmFamily::PingPongPersistent), (int)p.bnd, (int)p.dyn, (int)p.grouped, p.grid, p.splits,
         p.k_per_split);
  if (p.reduce != Reduce::None)
    printf(" | reduce %s %s %d",
           p.reduce == Reduce::Plain ? "plain" : p.reduce == Reduce::Transposed ? "t" : "grouped",
           p.slab == SlabType::BF16 ? "bf16" : "f32", p.splits);
  if (p.colsum) printf(" | colsum");
  putchar('\n');
}

int main(int argc, char** argv) {
  const int cus = argc > 1 ? atoi(argv[1]) : 256;
  char entry[32];
  while (scanf("%31s", entry) == 1) {
    int v[10];
    auto read = [&](int n) {
      for (int i = 0; i < n; ++i)
        if (scanf("%d", &v[i]) != 1) exit(2);
    };
    if (!strcmp(entry, "gemm")) {
      read(10);
      print_plan(plan_gemm(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8] != 0, v[9], cus));
    } else if (!strcmp(entry, "wgrad")) {
      read(7);
      print_plan(plan_wgrad(v[0], v[1], v[2], v[3], v[4], v[5], v[6], cus));
    } else if (!strcmp(entry, "wgrad_kt")) {
      read(5);
      print_plan(plan_wgrad_kt(v[0], v[1], v[2], v[3], v[4]));
    } else if (!strcmp(entry, "wgrad_grouped")) {
      read(1);
      const int count = v[0];
      int M[8], N[8];
      if (count < 0 || count > 8) return 2;
      for (int g = 0; g < count; ++g) {
        read(2);
        M[g] = v[0];
        N[g] = v[1];
      }
      read(3);
      print_plan(plan_wgrad_grouped(count, M, N, v[0], v[1], v[2]));
    } else {
      return 2;
    }
  }
  return 0;
}
