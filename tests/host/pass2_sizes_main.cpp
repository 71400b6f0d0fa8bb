// The LDS size functions of pass 2 on the CPU: shrimp_amd/csrc/gm_pass2_sizes.h (a header without HIP) decides which pass-2 kernel a read length gets and which window
// the mapping calls refuse.  For every read length on the command line, at the default window of 140 % (window_len_of of gm_host.hip), one line:
//   <read_len> <window> g4 <lds 4> <lds 8> cs <lds 1> <lds 4> <lds 8> max <letter space> <colour space> <colour space, local>
// tests/test_long_reads.py holds its restatement of the functions to these lines.
#include <cstdio>
#include <cstdlib>
#include "gm_pass2_sizes.h"

int main(int argc, char** argv) {
  printf("limit %zu\n", GM_SWF_LDS_LIMIT);
  for (int i = 1; i < argc; i++) {
    const int L = atoi(argv[i]);
    const double w = L * (140.0 / 100.0);
    const int W = (int)(uint16_t)w;
    printf("%d %d g4 %zu %zu cs %zu %zu %zu max %d %d %d\n", L, W, gm_pass2_g4_lds(4, L, W), gm_pass2_g4_lds(8, L, W), gm_pass2_cs_lds(1, L, W), gm_pass2_cs_lds(4, L, W),
           gm_pass2_cs_lds(8, L, W), gm_pass2_max_window(0, 0, L), gm_pass2_max_window(1, 0, L), gm_pass2_max_window(1, 1, L));
  }
  return 0;
}
