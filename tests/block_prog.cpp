// Stand-alone driver of the block cutter of a split range (pedn_plan::dead_block_len in pednstream_amd/csrc/pedn_plan.hpp), for
// tests/test_dead_block_host.py: no HIP, built with the host sanitizers.
//   block_prog T K_MAX W_MAX   for every t < t1 <= T, K <= K_MAX, W <= W_MAX (all from 1): one line "t t1 K W n1 n2 ..." -- the blocks that
//                              pedn_run cuts the steps [t, t1) into, in order
#include <stdio.h>
#include <stdlib.h>

#include "../pednstream_amd/csrc/pedn_plan.hpp"

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: block_prog T K_MAX W_MAX\n");
    return 2;
  }
  const int T = atoi(argv[1]), k_max = atoi(argv[2]), w_max = atoi(argv[3]);
  printf("max %d\n", pedn_plan::DEAD_BLOCK_MAX);
  for (int t0 = 1; t0 < T; ++t0)
    for (int t1 = t0 + 1; t1 <= T; ++t1)
      for (int K = 1; K <= k_max; ++K)
        for (int W = 1; W <= w_max; ++W) {
          printf("%d %d %d %d", t0, t1, K, W);
          int t = t0;
          while (t < t1) {   // (as pedn_run's loop over a split range)
            const int n = pedn_plan::dead_block_len(t, t1, K, W);
            printf(" %d", n);
            if (n < 1) return 1;   // (would not end)
            t += n;
          }
          printf("\n");
        }
  return 0;
}
