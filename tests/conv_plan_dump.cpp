// What drqv2_amd/csrc/conv_plan.h plans, one launch per input line, for tests/test_cpu_conv_variants.py to hold against
// tests/conv_variants.py.  Host only: the planner header is all it needs.  A line is
//   kind cus nb hin stride cin lay ws
// with kind conv_v (plan_conv_direct), wgrad (plan_wgrad_direct), wino (plan_wino), ww (plan_ww, dy the padded view the
// update passes; ww_flat: a contiguous dy), ww3 (plan_ww3), conv_bf16 (plan_conv_bf16), wgrad_bf16 (plan_wgrad_bf16),
// conv1_aug (plan_conv1_aug, `lay` riders) and reduce (plan_reduce of `nb` jobs: job 0 has `cin` channels, the others
// 32); ws = bytes of workspace per layer, -1: no limit; fields a kind does not use are ignored.
// Output: rc grid grid_y records[0..2] merged workspace-bytes-needed.
#include "../drqv2_amd/csrc/conv_plan.h"

#include <cstdio>
#include <cstring>

int main() {
  char kind[16];
  int cus, nb, hin, stride, cin, lay;
  long ws_in;
  while (std::scanf("%15s %d %d %d %d %d %d %ld", kind, &cus, &nb, &hin, &stride, &cin, &lay, &ws_in) == 8) {
    auto is = [&](const char* k) { return !std::strcmp(kind, k); };
    const size_t ws = ws_in < 0 ? ~(size_t)0 : (size_t)ws_in;
    const int cins[4] = {cin, 32, 32, 32};
    ConvPlan p;
    if (is("conv_v")) p = plan_conv_direct(cus, nb, hin, stride);
    else if (is("wgrad")) p = plan_wgrad_direct(cus, nb, cin, hin, stride, ws);
    else if (is("wino")) p = plan_wino(cus, nb, hin);
    else if (is("ww")) p = plan_ww(cus, nb, hin, ConvView::padded(hin - 2), ws);
    else if (is("ww_flat")) p = plan_ww(cus, nb, hin, ConvView::contiguous(hin - 2), ws);
    else if (is("ww3")) p = plan_ww3(cus, nb, ws);
    else if (is("conv_bf16")) p = plan_conv_bf16(cus, nb, hin, lay);
    else if (is("wgrad_bf16")) p = plan_wgrad_bf16(cus, nb, hin, ws);
    else if (is("conv1_aug")) p = plan_conv1_aug(cus, nb, lay);
    else if (is("reduce")) p = plan_reduce(nb, cins);
    else return 1;
    std::printf("%d %d %d %d %d %d %d %zu\n", p.rc, p.grid, p.grid_y, p.records[0], p.records[1], p.records[2],
                p.merged ? 1 : 0, p.ws_bytes);
  }
  return 0;
}
