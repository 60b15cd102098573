// Host program for the plain-C++ part of csrc/sgp_vfe_predict.hpp (built by g++ alone, with AddressSanitizer + UBSan, by
// tests/test_vfe_predict.py): the shape check of sgp_vfe_predict_batch with the order of its refusals, and the workspace query.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "sgp_vfe_predict.hpp"

using namespace sgp;

static int failures = 0;
#define EXPECT(c)                                             \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);      \
      ++failures;                                             \
    }                                                         \
  } while (0)

int main() {
  const int64_t P24 = int64_t(1) << 24;
  // the limits: sgp_vfe_eval_batch's, and sgp_predict's on T
  EXPECT(VP_MAXT == 32768 && VB_MAXM == 64 && VB_MAXN == 65536 && VB_MAXD == 8 && VB_MAXP == P24 - 1);
  EXPECT(vp_check(1, 1, 1, 1, 1, 0) == SGP_OK && vp_check(VB_MAXP, VB_MAXN, VB_MAXM, VB_MAXD, VP_MAXT, SGP_KERNEL_MATERN52) == SGP_OK);
  EXPECT(vp_check(2, 3, 5, 1, 7, SGP_KERNEL_MATERN32) == SGP_OK);  // M > N is legal
  // SGP_ERR_ARG: a count that is not positive, a kernel outside 0..2
  EXPECT(vp_check(0, 10, 5, 2, 7, 0) == SGP_ERR_ARG && vp_check(2, 0, 5, 2, 7, 0) == SGP_ERR_ARG && vp_check(2, 10, 0, 2, 7, 0) == SGP_ERR_ARG);
  EXPECT(vp_check(2, 10, 5, 0, 7, 0) == SGP_ERR_ARG && vp_check(2, 10, 5, 2, 0, 0) == SGP_ERR_ARG && vp_check(2, 10, 5, 2, -4, 0) == SGP_ERR_ARG);
  EXPECT(vp_check(2, 10, 5, 2, 7, -1) == SGP_ERR_ARG && vp_check(2, 10, 5, 2, 7, SGP_KERNEL_COMPOSITE) == SGP_ERR_ARG);
  // SGP_ERR_DIM: past a limit
  EXPECT(vp_check(2, 10, 65, 2, 7, 0) == SGP_ERR_DIM && vp_check(2, 65537, 5, 2, 7, 0) == SGP_ERR_DIM && vp_check(2, 10, 5, 9, 7, 0) == SGP_ERR_DIM);
  EXPECT(vp_check(P24, 10, 5, 2, 7, 0) == SGP_ERR_DIM && vp_check(2, 10, 5, 2, VP_MAXT + 1, 0) == SGP_ERR_DIM);
  EXPECT(vp_check(P24 - 1, 10, 5, 2, VP_MAXT, 0) == SGP_OK);
  // SGP_ERR_ARG comes before SGP_ERR_DIM, whichever argument carries which
  EXPECT(vp_check(0, 10, 65, 2, 7, 0) == SGP_ERR_ARG && vp_check(2, 10, 65, 2, 0, 0) == SGP_ERR_ARG);
  EXPECT(vp_check(2, 10, 5, 2, VP_MAXT + 1, SGP_KERNEL_COMPOSITE) == SGP_ERR_ARG && vp_check(2, 10, 65, 2, VP_MAXT + 1, -1) == SGP_ERR_ARG);
  EXPECT(vp_check(0, 10, 5, 2, VP_MAXT + 1, 0) == SGP_ERR_ARG);
  // the workspace placeholder: one aligned unit for a supported shape, nothing otherwise
  EXPECT(vp_workspace_bytes(1, 1, 1, 1, 1) == VB_WS_UNIT && VB_WS_UNIT == WG_WS_UNIT && VB_WS_UNIT % 256 == 0);
  EXPECT(vp_workspace_bytes(VB_MAXP, VB_MAXN, VB_MAXM, VB_MAXD, VP_MAXT) == VB_WS_UNIT);
  EXPECT(vp_workspace_bytes(2, 10, 65, 2, 7) == 0 && vp_workspace_bytes(0, 10, 5, 2, 7) == 0 && vp_workspace_bytes(2, 65537, 5, 2, 7) == 0);
  EXPECT(vp_workspace_bytes(P24, 10, 5, 2, 7) == 0 && vp_workspace_bytes(2, 10, 5, 9, 7) == 0);
  EXPECT(vp_workspace_bytes(2, 10, 5, 2, 0) == 0 && vp_workspace_bytes(2, 10, 5, 2, VP_MAXT + 1) == 0);
  // the test stage's geometry: Mp / 8 lanes per test point cover the 256 threads once, eight entries of a row each
  for (int Mp : {16, 32, 64}) {
    const int tn = vb_tile_rows(Mp), tpp = Mp / 8;
    EXPECT(tpp * tn == 256 && tpp * 8 == Mp && 64 % tpp == 0 && (tpp & (tpp - 1)) == 0);
  }
  if (failures) return 1;
  std::printf("vfe predict host ok\n");
  return 0;
}
