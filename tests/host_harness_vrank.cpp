// TEST INFRASTRUCTURE ONLY: the host-side arithmetic of ld_vrank_reduce
// (ld::vrank_mean of ld_amd/csrc/ld_math.h, the function the gfx950 kernel calls
// once per column) compiled with g++, so the CPU test-suite can check the
// ascending-order fp32 sum and the single division without a GPU.  The product
// never links or loads this.
#include "../ld_amd/csrc/ld_math.h"

extern "C" {
// out[c] = mean over the W rows of column c of a (W, n) table with row_stride
// floats between rows: the kernel's loop over columns, one "thread" at a time
void h_vrank_reduce(const float* table, int W, int n, size_t row_stride, float* out) {
  for (int c = 0; c < n; ++c) out[c] = ld::vrank_mean(table + c, W, row_stride);
}
}
