// pf_strip_map.h -- which lane moves which 16 bytes of a column strip's tile (pf_wall.h: the staged strip bodies).
//
// A column-strip block (k_wall2, MODE 2) holds a tile of 64 rows (the lanes, along y) x DP cells (the pencil, along z), NV = DP / V vectors
// per row.  In the per-lane form a lane loads and stores its own pencil: every instruction touches 64 rows, one memory line each.  The staged
// form issues the SAME addresses with another lane assignment -- instruction i, lane l moves element e = 64 i + l of the tile, counted row
// by row, so consecutive lanes move consecutive 16 bytes of one row -- and exchanges the vectors through a tile in LDS:
//
//   loads:  element e = vector e % NV of row e / NV, from the row's own source row (strip_lane_src: the clamp and the ghost mirror of the
//           per-lane rule, computed for that row), written to LDS at strip_lds_elem(e), read by lane L, vector v at strip_lds_pencil(L, v, NV);
//   stores: lane L writes its owned vectors q0 .. q0 + NVo - 1 at strip_lds_pencil(L, q, NV); element e = vector q0 + e % NVo of row e / NVo is
//           read from there and stored where the row is owned (strip_row_owned: the per-lane rule's own_lane, for that row).
//
// fp32, DP = 20: rows of 80 bytes.  A 16-byte LDS access is served sixteen lanes at a time; sixteen lanes at a stride of 80 bytes start in
// sixteen different 16-byte groups of the 256 bytes the banks span (20 L mod 64 words takes every multiple of 4 once): no padding, no conflicts.
//
// Nothing here touches a device: tests/strip_map_check.cpp checks the maps against the per-lane rules on the CPU.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PF_STRIP_HD __host__ __device__
#else
#define PF_STRIP_HD
#endif

namespace pf {

constexpr int STRIP_ROWS = 64; // rows of a tile = lanes of the wave

// element -> (row, vector) with nv vectors per row
PF_STRIP_HD constexpr int strip_row(int e, int nv) { return (int)((unsigned)e / (unsigned)nv); }
PF_STRIP_HD constexpr int strip_vec(int e, int nv) { return (int)((unsigned)e % (unsigned)nv); }
// the element instruction i hands to lane l
PF_STRIP_HD constexpr int strip_elem(int i, int lane) { return STRIP_ROWS * i + lane; }
// coordinate of tile row `row` on the lane axis: the tile starts hl rows before the lt rows tile j owns
PF_STRIP_HD constexpr int strip_row_coord(int row, int l0, int hl, int lt, int j) { return l0 - hl + lt * j + row; }
// where a row's u^n comes from (wall_body: lsrc): clamped into the grid, a ghost row (0, NL - 1) takes the row two inside.  As two reflections --
// about row 1, then about row NL - 2; each moves the ghost row alone --: no compare and select per row (NL >= 4)
PF_STRIP_HD constexpr int strip_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
PF_STRIP_HD constexpr int strip_abs(int x) { return x < 0 ? -x : x; }
PF_STRIP_HD constexpr int strip_lane_src(int lc, int NL) { return NL - 2 - strip_abs(NL - 3 - strip_abs(strip_clamp(lc, 0, NL - 1) - 1)); }
// does the tile own the row (wall_body: own_lane = row >= hl && row <= 63 - hl && its coordinate < l1)?  The owned rows are hl .. hl + n - 1 with n the
// count below (wave-uniform, once per block): one unsigned compare per row
PF_STRIP_HD constexpr int strip_owned_rows(int tl0, int hl, int l1) { return strip_clamp(l1 - (tl0 + hl), 0, STRIP_ROWS - 2 * hl); } // tl0: coordinate of row 0
PF_STRIP_HD constexpr bool strip_row_owned(int row, int hl, int nown) { return (unsigned)(row - hl) < (unsigned)nown; }
// the vectors of a pencil a store writes (store_pencil: (q + 1) V > ko0 && q V < ko1): the first, and how many
PF_STRIP_HD constexpr int strip_q0(int ko0, int V) { return ko0 / V; }
PF_STRIP_HD constexpr int strip_nvo(int ko0, int ko1, int V) { return (ko1 + V - 1) / V - ko0 / V; }
// places in the LDS tile, in vectors: element e in the rows' order (= its number: row-major, like the pencils'); vector v of row / lane L's pencil; the tile's size
PF_STRIP_HD constexpr int strip_lds_elem(int e) { return e; }
PF_STRIP_HD constexpr int strip_lds_pencil(int lane, int v, int nv) { return nv * lane + v; }
PF_STRIP_HD constexpr int strip_lds_vectors(int nv) { return STRIP_ROWS * nv; }

} // namespace pf
