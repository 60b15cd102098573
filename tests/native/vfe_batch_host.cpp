// Host program for the plain-C++ part of csrc/sgp_vfe_batch.hpp (built by g++ alone, with AddressSanitizer + UBSan, by
// tests/test_vfe_batch.py): the size class of M, the tile geometry, the refusals and their order, the workspace query and the theta-row
// check.  The arrays handed to vb_theta_ok are heap blocks of exactly the length it may read.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sgp_vfe_batch.hpp"

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
  // size classes: 16 | 32 | 64, none outside 1..64
  for (int M = -3; M <= 70; ++M) {
    const int c = vb_size_class(M);
    if (M < 1 || M > 64) EXPECT(c == 0);
    else EXPECT(c == (M <= 16 ? 16 : M <= 32 ? 32 : 64) && c >= M && c % 16 == 0);
  }
  // the tile geometry the kernel is written from: 8 entries per thread in every class, whole 16-row blocks, the tiles cover the rows
  // and the last one is not empty
  EXPECT(vb_tile_rows(16) == 128 && vb_tile_rows(32) == 64 && vb_tile_rows(64) == 32);
  const int Ns[] = {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 257, 1984, 1985, 2049, 65535, 65536};
  for (int Mp : {16, 32, 64}) {
    const int tn = vb_tile_rows(Mp), tpr = vb_threads_per_row(Mp);
    EXPECT(tn * Mp == VB_TILE_ENTRIES && tn * Mp == 256 * 8 && tn % 16 == 0 && tpr * Mp == 256 && tn == 8 * tpr && 64 % tpr == 0);
    for (int N : Ns) {
      const int nt = vb_tiles(N, Mp);
      EXPECT(nt >= 1 && nt * tn >= N && (nt - 1) * tn < N);
    }
  }
  // refusals: SGP_ERR_ARG before SGP_ERR_DIM
  EXPECT(vb_check(1, 1, 1, 1, 0) == SGP_OK && vb_check(VB_MAXP, VB_MAXN, VB_MAXM, VB_MAXD, SGP_KERNEL_MATERN52) == SGP_OK);
  EXPECT(vb_check(0, 10, 5, 2, 0) == SGP_ERR_ARG && vb_check(2, 0, 5, 2, 0) == SGP_ERR_ARG && vb_check(2, 10, 0, 2, 0) == SGP_ERR_ARG);
  EXPECT(vb_check(2, 10, 5, 0, 0) == SGP_ERR_ARG && vb_check(2, 10, 5, 2, -1) == SGP_ERR_ARG);
  EXPECT(vb_check(2, 10, 5, 2, SGP_KERNEL_COMPOSITE) == SGP_ERR_ARG && vb_check(2, 10, 65, 2, SGP_KERNEL_COMPOSITE) == SGP_ERR_ARG);
  EXPECT(vb_check(2, 10, 65, 2, 0) == SGP_ERR_DIM && vb_check(2, 65537, 5, 2, 0) == SGP_ERR_DIM && vb_check(2, 10, 5, 9, 0) == SGP_ERR_DIM);
  EXPECT(vb_check(int64_t(1) << 24, 10, 5, 2, 0) == SGP_ERR_DIM && vb_check((int64_t(1) << 24) - 1, 10, 5, 2, 0) == SGP_OK);
  EXPECT(vb_check(0, 10, 65, 2, 0) == SGP_ERR_ARG);
  // the workspace placeholder: one aligned unit for a supported shape, nothing otherwise
  EXPECT(vb_workspace_bytes(1, 1, 1, 1) == VB_WS_UNIT && VB_WS_UNIT % 256 == 0);
  EXPECT(vb_workspace_bytes(VB_MAXP, VB_MAXN, VB_MAXM, VB_MAXD) == VB_WS_UNIT);
  EXPECT(vb_workspace_bytes(2, 10, 65, 2) == 0 && vb_workspace_bytes(0, 10, 5, 2) == 0 && vb_workspace_bytes(2, 65537, 5, 2) == 0);
  EXPECT(vb_workspace_bytes(int64_t(1) << 24, 10, 5, 2) == 0 && vb_workspace_bytes(2, 10, 5, 9) == 0);
  // theta rows
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double bad[] = {nan, 0.0, -0.0, -0.3, inf, -inf};
  for (int n = 3; n <= VB_MAXD + 2; ++n) {
    std::vector<double>* row = new std::vector<double>(n, 1.25);   // exactly n doubles on the heap
    EXPECT(vb_theta_ok(row->data(), n));
    (*row)[0] = std::numeric_limits<double>::denorm_min();
    (*row)[n - 1] = std::numeric_limits<double>::max();
    EXPECT(vb_theta_ok(row->data(), n));
    for (double b : bad) {
      for (int at : {0, n / 2, n - 1}) {
        std::vector<double> r(n, 0.7);
        r[at] = b;
        EXPECT(!vb_theta_ok(r.data(), n));
      }
    }
    delete row;
  }
  if (failures) return 1;
  std::printf("vfe batch host ok\n");
  return 0;
}
