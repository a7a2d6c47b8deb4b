// Host build of the plain-C++ part of csrc/gridscan.h (grid fit, cell index) for tests/test_gridfit_cpu.py (test
// infrastructure, g++ only).
#include "../humangaussian_amd/csrc/gridscan.h"
extern "C" float hgs_grid_volume_host(const float* ext, float emax) { return hgs_grid_volume(ext, emax); }
// g[3] out; returns h
extern "C" float hgs_grid_fit_host(const float* ext, float h0, uint32_t nc_max, uint32_t* g) { return hgs_grid_fit(ext, h0, nc_max, g); }
extern "C" void hgs_grid_cell1_host(int n, const float* x, float origin, float inv_h, int g, int32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = hgs_grid_cell1(x[i], origin, inv_h, g);
}
