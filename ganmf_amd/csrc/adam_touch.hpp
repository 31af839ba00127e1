// Index arithmetic shared by the GEMM kernels and a host program (tests/adam_touch_walk.cpp): plain C++, no HIP types.
//
//   * block id -> tile of a one-tile-per-workgroup GEMM (list order, column-fastest order, XCD-blocked order);
//   * the early touch of the fused-Adam epilogue: which dword of theta / m / v a thread of a tile's workgroup loads in front of the
//     K loop.  The row pass behind the K loop (gemm_f32.hpp, gemm_epilogue) reads rows m0 .. m0 + BM - 1 below M and, of each, the
//     columns n0 .. n0 + BN - 1 below N of the three arrays.  Leading dimensions are multiples of 64 floats and n0 of BN, so a tile row
//     of one array is BN / 32 whole 128-byte lines.  A slot is one such line: the touch loads its first dword, and only where the row
//     pass itself reads that dword (row < M, column < N) -- an out-of-range touch is the one way the touch could fault, and the host
//     program walks every tile and thread to show there is none.
#pragma once

#if defined(__HIPCC__)
#define GANMF_HD __host__ __device__
#else
#define GANMF_HD
#endif

namespace ganmf {

GANMF_HD inline int xcd_remap(int bid, int nwg) {
  // blocks b and b+8 share an XCD (observed round-robin dispatch; speed only, never correctness)
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

GANMF_HD inline int part_begin(int n, int parts, int i) { return (int)(((long long)n * i) / parts); }

// the tile grid and the order its tiles are handed out in (GemmP's fields of the same names)
struct TileGrid { int tiles_m, tiles_n, nsplit, xb_m, xb_n, xb_band, n_fastest; };

// block id -> (tile row, tile column, K split, batch).  Default: list order, tm fastest, each XCD a contiguous range of the
// list.  xb_m > 0: the list is re-ordered rectangle by rectangle (rectangle r = (r % xb_m, r / xb_m) of the tile grid),
// inside a rectangle band by band, inside a band M-innermost; XCD x still takes a contiguous range of the list, i.e. its own
// rectangle up to a few tiles of drift where the rectangles' sizes differ.  Bijective for every shape.
GANMF_HD inline void tile_order(const TileGrid& g, int bid, int nblk, int& tm, int& tn, int& sp, int& bz) {
  int t = xcd_remap(bid, nblk);
  if (g.xb_m > 0) {
    sp = 0; bz = 0;
    int mb0 = 0, nb0 = 0, bm = 1, bn = 1;
    for (int r = 0; r < 8; ++r) {
      const int i = r % g.xb_m, j = r / g.xb_m;
      mb0 = part_begin(g.tiles_m, g.xb_m, i); bm = part_begin(g.tiles_m, g.xb_m, i + 1) - mb0;
      nb0 = part_begin(g.tiles_n, g.xb_n, j); bn = part_begin(g.tiles_n, g.xb_n, j + 1) - nb0;
      if (t < bm * bn) break;
      t -= bm * bn;
    }
    const int bx = g.xb_band > 1 ? g.xb_band : 1;
    const int bh = bx < bm ? bx : bm;               // band height in tiles
    const int band = t / (bh * bn);
    const int r = t - band * bh * bn;
    const int rest = bm - band * bh;
    const int h = bh < rest ? bh : rest;            // the last band of a rectangle may be shorter
    tm = mb0 + band * bh + r % h;
    tn = nb0 + r / h;
    return;
  }
  if (g.n_fastest) {
    tn = t % g.tiles_n; t /= g.tiles_n;
    tm = t % g.tiles_m; t /= g.tiles_m;
  } else {
    tm = t % g.tiles_m; t /= g.tiles_m;
    tn = t % g.tiles_n; t /= g.tiles_n;
  }
  sp = t % g.nsplit;
  bz = t / g.nsplit;
}

// ---- early touch of the Adam streams
constexpr int ADAM_TOUCH_LINE = 32;      // floats of a 128-byte line

// slots of a BM x BN tile: three arrays x BM rows x BN / 32 lines, array-major, then row-major (consecutive threads take
// consecutive lines of one array)
constexpr int adam_touch_slots(int bm, int bn) { return 3 * bm * (bn / ADAM_TOUCH_LINE); }

struct AdamTouch {
  int arr;             // 0 theta, 1 m, 2 v; -1: the slot lies outside the tensor, nothing is loaded
  long long off;       // element offset from the array's base: row * ld + column
};

GANMF_HD inline AdamTouch adam_touch_slot(int bm, int bn, int slot, int m0, int n0, int M, int N, int ld) {
  const int lpr = bn / ADAM_TOUCH_LINE, per = bm * lpr;
  const int arr = slot / per, s = slot - arr * per;
  const int row = m0 + s / lpr, col = n0 + (s % lpr) * ADAM_TOUCH_LINE;
  if (arr > 2 || row >= M || col >= N) return AdamTouch{-1, 0};
  return AdamTouch{arr, (long long)row * ld + col};
}

}  // namespace ganmf
