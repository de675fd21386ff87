// Which workgroup computes which output tile: the XCD-aware orders of the GEMM and LSTM-step kernels, as pure integer functions of
// the block index and the grid.  The dispatcher deals blocks round-robin over the 8 XCDs (blocks b and b + 8 share one, b % 8 names
// the group, not the XCD); each order hands one XCD's blocks tiles that share operand panels, so those panels stay in that XCD's L2.
// Placement is a matter of speed only: every map here is a bijection from blocks onto tiles at every grid, whatever the dispatcher
// does.  tests/test_tile_order_cpu.py compiles this header as host C++ and enumerates each map.
#pragma once

// Block id of n -> work unit: each XCD takes a contiguous run of n / 8 units (n % 8 == 0; otherwise the identity).
__host__ __device__ inline int xcd_order(int id, int n) { return (n & 7) == 0 ? (id & 7) * (n >> 3) + (id >> 3) : id; }

struct TileMN {
  int m, n;     // row panel, column tile
};

// ---- 320 x 256 tiles, one workgroup per CU (gemm_tile_big_kernel, s3_gemm_big_kernel) ------------------------------------------
// The panel walk: XCD x (blocks x, x + 8, ...) takes blocks of 4 row panels x 8 column tiles, 32 blocks of it per round, so its A
// panels stay in its L2 for a round.  It maps the n blocks one-to-one onto the tiles only when every XCD runs whole rounds (n % 256 ==
// 0) and the blocks tile the grid (tiles_m % 4 == 0, tiles_n % 8 == 0); elsewhere each kernel keeps its linear order.
__host__ __device__ inline bool panel_walk_fits(int n, int tiles_m, int tiles_n) {
  return n % 256 == 0 && tiles_m % 4 == 0 && tiles_n % 8 == 0;
}

// Block b of n on the walk over tiles_n column tiles; the row panels of several batch entries count on as one column of panels.
__host__ __device__ inline TileMN panel_walk(int b, int n, int tiles_n) {
  const int blk = (b & 7) * (n >> 8) + (b >> 8), within = (b >> 3) & 31;     // block of 4 x 8 tiles, position inside it
  const int nb_n = tiles_n >> 3;
  return {(blk / nb_n) * 4 + (within & 3), (blk % nb_n) * 8 + (within >> 2)};
}

// gemm_tile_big_kernel: nbatch x tiles_m x tiles_n tiles on n = nbatch tiles_m tiles_n blocks; row-major where the walk does not fit.
// m counts the row panels of all batch entries: batch = m / tiles_m.
__host__ __device__ inline TileMN panel_walk_or_row_major(int b, int n, int tiles_m, int tiles_n) {
  return panel_walk_fits(n, tiles_m, tiles_n) ? panel_walk(b, n, tiles_n) : TileMN{b / tiles_n, b % tiles_n};
}

// s3_gemm_big_kernel: tiles_m x tiles_n tiles on n = tiles_m tiles_n blocks; column-major where the walk does not fit.
__host__ __device__ inline TileMN panel_walk_or_col_major(int b, int n, int tiles_m, int tiles_n) {
  return panel_walk_fits(n, tiles_m, tiles_n) ? panel_walk(b, n, tiles_n) : TileMN{b % tiles_m, b / tiles_m};
}

// ---- persistent grids (lstm_step_bf16_fused256_kernel) ------------------------------------------------------------------------
// Workgroup b of G, iteration it -> tile; tiles rise with it, and the workgroup stops at the first one >= ntiles.  With 8 x 32
// workgroups and tiles that divide evenly, XCD x takes a contiguous run of ntiles / 8 tiles, 32 at a time; otherwise workgroup b takes
// tiles b, b + G, ...
__host__ __device__ inline int persistent_tile(int b, int it, int G, int ntiles) {
  return G == 256 && ntiles % 256 == 0 ? (b & 7) * (ntiles >> 3) + it * 32 + (b >> 3) : b + it * G;
}
