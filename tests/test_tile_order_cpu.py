"""The tile orders of mmego_amd/csrc/tile_order.h, enumerated on the CPU: the header is compiled as host C++ (g++, __host__ and
__device__ defined away) into a program that walks every block of every grid below and counts, per tile, the blocks that compute it.
Each map must be a bijection from blocks onto tiles, fallback orders included."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmego_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "tile_order.h"

static std::vector<int> hits;
static long shapes = 0, bad = 0;

static void reset(int tiles) { hits.assign(tiles, 0); }
static bool hit(int tile) {
  if (tile < 0 || tile >= (int)hits.size()) return false;
  return ++hits[tile] == 1;
}
static void done(const char* map, bool ok, int a, int b, int c, int d) {
  for (int h : hits) ok = ok && h == 1;
  ++shapes;
  if (!ok && bad++ < 5) std::printf("FAIL %s %d %d %d %d\n", map, a, b, c, d);
}

int main() {
  for (int n = 1; n <= 8192; ++n) {
    reset(n);
    bool ok = true;
    for (int b = 0; b < n; ++b) ok = hit(xcd_order(b, n)) && ok;
    done("xcd_order", ok, n, 0, 0, 0);
  }
  for (int tm = 1; tm <= 64; ++tm)
    for (int tn = 1; tn <= 64; ++tn) {
      for (int nbatch = 1; nbatch <= 4; ++nbatch) {
        const int n = nbatch * tm * tn;
        reset(n);
        bool ok = true;
        for (int b = 0; b < n; ++b) {
          const TileMN t = panel_walk_or_row_major(b, n, tm, tn);
          ok = t.n >= 0 && t.n < tn && hit(t.m * tn + t.n) && ok;     // t.m: row panel over the batch entries
        }
        done("panel_walk_or_row_major", ok, tm, tn, nbatch, 0);
      }
      const int n = tm * tn;
      reset(n);
      bool ok = true;
      for (int b = 0; b < n; ++b) {
        const TileMN t = panel_walk_or_col_major(b, n, tm, tn);
        ok = t.n >= 0 && t.n < tn && hit(t.m * tn + t.n) && ok;
      }
      done("panel_walk_or_col_major", ok, tm, tn, 1, 0);
    }
  const int grids[] = {1, 7, 8, 100, 128, 255, 256, 257, 512};
  for (int G : grids)
    for (int ntiles = 1; ntiles <= 4096; ++ntiles) {
      reset(ntiles);
      bool ok = true;
      const int niter = (ntiles + G - 1) / G;
      for (int b = 0; b < G; ++b)
        for (int it = 0; it < niter; ++it) {                             // as lstm_step_bf16_fused256_kernel walks it
          const int tile = persistent_tile(b, it, G, ntiles);
          if (tile >= ntiles) break;
          ok = hit(tile) && ok;
        }
      done("persistent_tile", ok, G, ntiles, 0, 0);
    }
  std::printf("shapes %ld bad %ld\n", shapes, bad);
  return 0;
}
"""


def test_every_tile_order_is_a_bijection_from_blocks_onto_tiles(tmp_path):
    src, exe = tmp_path / "tile_order.cpp", tmp_path / "tile_order"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__host__=", "-D__device__=", "-I", CSRC, "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=300).stdout
    assert "FAIL" not in out, out
    # 8192 xcd_order grids, 64 x 64 x (4 + 1) panel-walk grids, 9 x 4096 persistent grids
    assert out.split()[-4:] == ["shapes", str(8192 + 64 * 64 * 5 + 9 * 4096), "bad", "0"], out
