// Host walk of the early touch of the Adam streams (ganmf_amd/csrc/adam_touch.hpp), built by tests/test_adam_touch_walk.py with
// -fsanitize=address,undefined.  For every product it is given it allocates theta / m / v at exactly M * ld floats, runs every block and
// thread of the launch through the kernel's own index arithmetic (tile_order, adam_touch_slot), READS every touched element (so the
// sanitizer sees an access outside the allocation as well as the explicit range check) and compares with a model of the row pass of
// gemm_epilogue (64 x 64 tile, one float4 per thread and row step, rows below M, columns below N), for workgroups of 256, 512 and 1024
// threads (the fp32 ring kernel's one, two or four K groups):
//   * every block id maps to a tile of the grid, every tile is visited once;
//   * every touched offset lies in [0, M * ld) and is an element the row pass reads;
//   * every 128-byte line the row pass reads is touched exactly once, no other line is touched.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ganmf_amd/csrc/adam_touch.hpp"

using namespace ganmf;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s: ", what); std::printf(__VA_ARGS__); std::printf("\n"); if (++g_fail > 20) std::exit(1); } } while (0)

static int round_up(int x, int a) { return (x + a - 1) / a * a; }

// one fused-Adam product: C is [M, N] with leading dimension ld, tiles in the order `g` gives; nthr threads per workgroup
static void walk(const char* what, int M, int N, int ld, TileGrid g, int nthr) {
  constexpr int BM = 64, BN = 64;
  g.tiles_m = (M + BM - 1) / BM; g.tiles_n = (N + BN - 1) / BN; g.nsplit = 1;
  const long long elems = (long long)M * ld;
  const long long lines = elems / ADAM_TOUCH_LINE;
  CHECK(ld % 64 == 0 && ld >= N, "leading dimension %d", ld);
  float* base[3];
  for (int a = 0; a < 3; ++a) { base[a] = new float[elems]; for (long long i = 0; i < elems; ++i) base[a][i] = 1.f; }
  std::vector<int> touched[3];
  for (int a = 0; a < 3; ++a) touched[a].assign(lines, 0);
  std::vector<char> read(elems, 0);
  std::vector<int> seen((size_t)g.tiles_m * g.tiles_n, 0);
  const int nblk = g.tiles_m * g.tiles_n;
  const int nr = (adam_touch_slots(BM, BN) + nthr - 1) / nthr;
  double sum = 0;
  for (int bid = 0; bid < nblk; ++bid) {
    int tm = -1, tn = -1, sp = -1, bz = -1;
    tile_order(g, bid, nblk, tm, tn, sp, bz);
    CHECK(tm >= 0 && tm < g.tiles_m && tn >= 0 && tn < g.tiles_n && sp == 0 && bz == 0, "block %d -> tile (%d, %d) split %d batch %d", bid, tm, tn, sp, bz);
    if (!(tm >= 0 && tm < g.tiles_m && tn >= 0 && tn < g.tiles_n)) continue;
    ++seen[(size_t)tn * g.tiles_m + tm];
    const int m0 = tm * BM, n0 = tn * BN;
    // the row pass: C4 = 16 float4 per tile row, RPP rows per step
    const int c4 = BN / 4, rpp = nthr / c4 < BM ? nthr / c4 : BM;
    for (int tid = 0; tid < nthr; ++tid) {
      const int tc = tid % c4, tr = tid / c4, col = n0 + 4 * tc;
      for (int j = 0; j < BM / rpp; ++j) {
        const int row = m0 + tr + j * rpp;
        if (tr + j * rpp >= BM || row >= M || col >= N) continue;
        for (int q = 0; q < 4 && col + q < N; ++q) read[(long long)row * ld + col + q] = 1;
      }
    }
    for (int tid = 0; tid < nthr; ++tid)
      for (int j = 0; j < nr; ++j) {
        const AdamTouch t = adam_touch_slot(BM, BN, j * nthr + tid, m0, n0, M, N, ld);
        if (t.arr < 0) continue;
        CHECK(t.arr <= 2, "array %d", t.arr);
        CHECK(t.off >= 0 && t.off < elems, "tile (%d, %d) thread %d: offset %lld outside [0, %lld)", tm, tn, tid, t.off, elems);
        if (t.arr > 2 || t.off < 0 || t.off >= elems) continue;
        sum += base[t.arr][t.off];
        CHECK(read[t.off], "tile (%d, %d) thread %d touches element %lld, which the row pass does not read", tm, tn, tid, t.off);
        ++touched[t.arr][t.off / ADAM_TOUCH_LINE];
      }
  }
  for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "tile %zu visited %d times", i, seen[i]);
  long long nread = 0;
  for (long long l = 0; l < lines; ++l) {
    bool any = false;
    for (int q = 0; q < ADAM_TOUCH_LINE; ++q) any = any || read[l * ADAM_TOUCH_LINE + q];
    nread += any;
    for (int a = 0; a < 3; ++a) CHECK(touched[a][l] == (any ? 1 : 0), "array %d line %lld: read %d, touched %d times", a, l, (int)any, touched[a][l]);
  }
  CHECK(sum == 3.0 * (double)nread, "touched %.0f elements, expected %lld", sum, 3 * nread);
  std::printf("ok   %-40s M %5d N %5d ld %5d  %4d tiles x %4d threads  %lld lines per array\n", what, M, N, ld, nblk, nthr, nread);
  for (int a = 0; a < 3; ++a) delete[] base[a];
}

// gV of the generator step (the product that carries the touch) and the two weight-gradient products of a GANMF discriminator step plus
// DisGANMF's W_0 (the same epilogue; the host leaves their flag off where the state is large), in the tile orders the step uses
static void ganmf_shape(const char* name, int N, int k, int e) {
  char what[128];
  const TileGrid list{0, 0, 1, 0, 0, 0, 0}, nfast{0, 0, 1, 0, 0, 0, 1};
  for (int nthr : {256, 512, 1024}) {
    std::snprintf(what, sizeof what, "%s gV", name);
    walk(what, N, k, round_up(k + 1, 64), nthr == 512 ? list : nfast, nthr);
    std::snprintf(what, sizeof what, "%s gWd_ext xb %d", name, nthr == 256 ? 16 : nthr == 512 ? 2 : 1);
    walk(what, e + 1, N, round_up(N + 2, 64), TileGrid{0, 0, 1, 1, 8, nthr == 256 ? 16 : nthr == 512 ? 2 : 1, 0}, nthr);
    std::snprintf(what, sizeof what, "%s gWe_ext", name);
    walk(what, N + 1, e, round_up(e + 1, 64), nfast, nthr);
  }
  std::snprintf(what, sizeof what, "%s gWd_ext list order", name);
  walk(what, e + 1, N, round_up(N + 2, 64), list, 256);
  std::snprintf(what, sizeof what, "%s W_0 (N + 2 rows)", name);
  walk(what, N + 2, e, round_up(e + 1, 64), nfast, 1024);
}

int main() {
  ganmf_shape("(70, 65, 5, 33, 16)", 65, 5, 33);
  ganmf_shape("(96, 129, 8, 64, 32)", 129, 8, 64);
  ganmf_shape("(64, 63, 4, 7, 32)", 63, 4, 7);
  ganmf_shape("ML-1M (6040, 3706, 250, 992, 128)", 3706, 250, 992);
  ganmf_shape("(300, 300, 16, 70, 64): empty rectangles", 300, 16, 70);      // 5 tile columns of gWd over 8 XCD rectangles
  ganmf_shape("(200, 65, 5, 33, 96)", 65, 5, 33);
  ganmf_shape("(150, 129, 70, 64, 80)", 129, 70, 64);
  if (g_fail) { std::printf("%d failures\n", g_fail); return 1; }
  std::printf("all walks clean\n");
  return 0;
}
