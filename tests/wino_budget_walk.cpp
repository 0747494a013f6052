// Host walk of a budgeted conv3x3_wino_kernel launch for tests/test_cpu_wino_budget.py: the grid plan_wino gives and,
// wave by wave, what wino_deal (drqv2_amd/csrc/conv_plan.h, the function the kernel decodes its work with) hands out.
// Host only: the planner header is all it needs.  A line is
//   cus nb hin budget
// Output per line:
//   grid grid_unbudgeted nunit once other stray most least
// once = (unit, channel half) pairs owned by exactly one wave, other = pairs owned by none or by several, stray = items
// handed out beyond [0, nunit), most / least = the largest / smallest load of a wave in half-units.
#include "../drqv2_amd/csrc/conv_plan.h"

#include <cstdio>
#include <vector>

int main() {
  int cus, nb, hin, budget;
  while (std::scanf("%d %d %d %d", &cus, &nb, &hin, &budget) == 4) {
    const ConvPlan p = plan_wino(cus, nb, hin, budget), p0 = plan_wino(cus, nb, hin);
    const int nunit = (int)wino_units(nb, hin);
    std::vector<int> owners(2 * (size_t)nunit, 0);
    long stray = 0;
    int most = 0, least = 1 << 30;
    for (int b = 0; b < p.grid; ++b)
      for (int w = 0; w < 4; ++w) {
        const WinoDeal d = wino_deal(p.grid, b, w, nunit);
        auto own = [&](int unit, int h) {
          if (unit < 0 || unit >= nunit) ++stray;
          else ++owners[2 * (size_t)unit + h];
        };
        for (int i = 0; i < d.nfull; ++i) {
          own(d.gw + i * d.nwave, 0);
          own(d.gw + i * d.nwave, 1);
        }
        if (d.has_half) own(d.half_unit, d.half_h);
        const int load = 2 * d.nfull + (d.has_half ? 1 : 0);
        if (load > most) most = load;
        if (load < least) least = load;
      }
    long once = 0, other = 0;
    for (int o : owners) (o == 1 ? once : other) += 1;
    std::printf("%d %d %d %ld %ld %ld %d %d\n", p.grid, p0.grid, nunit, once, other, stray, most, least);
  }
  return 0;
}
