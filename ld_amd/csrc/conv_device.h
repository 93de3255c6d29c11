// Device-side pieces shared by the bf16 forward / data-gradient conv kernels of
// conv_bf16.hip and conv_t256.hip: the vector types, the 16-byte
// buffer load and the ONE epilogue of the four kernels.  conv_common.h keeps the
// structs, the gather geometry and the host hooks.
#pragma once
#include "conv_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float floatx8 __attribute__((ext_vector_type(8)));
typedef float floatx4_t __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uintx4 buf_load16(rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(uintx4,
                            __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

}  // namespace

// Epilogue of the bf16 kernels for a wave tile of TM x TN accumulator tiles whose
// first row / column are ROW_FIRST / COL_FIRST: direct stores, 32 consecutive
// positions per accumulator row.  Expands in a kernel's scope and uses its `a`,
// `acc`, `Cout`, `l31`, `lk`, `MODE`, `TM`, `TN`.
//   * Loop order: row group g = 4 accumulator rows (one C8 half-row) x all TN
//     column tiles; every load of a group -- affine, bias, fp32 / C8 residual --
//     is issued before the group's first store.  The pointers of ConvK may alias
//     as far as hipcc knows, so a residual load written between stores stays
//     behind the previous store: the loop this replaces made up to 16 dependent
//     round trips per 32 x 32 tile, each waited for with vmcnt(0) (ISA reading;
//     the 256 -> 1024 expansion convs ran at 1.2 TB/s).
//   * Per-channel operands go through descriptors: an absent one has extent 0 and
//     loads as 0 -- no flag-dependent branch inside a group's load phase.
//   * Group fence (the sched_barrier): the loads of a group stay behind the
//     previous group's stores and none of them is consumed before all are issued.
//   * C8 images (side output, residual) exist for MODE 0 only: compact position.
//     Side output a.y_c8 = the bf16 channel-blocked image of y, for the conv that
//     consumes y next.  A lane holds rows row0 .. row0 + 3 of one position: four
//     consecutive channels = one half of a 16-byte C8 row -> one 8-byte store
//     (c8row = byte offset of that half within an image); the two lane halves of
//     a wave fill the row, consecutive lanes consecutive positions (coalesced).
//   * RAWC8 (the C8-input kernels): a.raw_c8, the conv result before the affine
//     as a C8 image -- what the BN backward reads for d(gamma), 2 instead of 4
//     bytes per element.
// A macro, not a function: hipcc optimises an inline function on its own before
// it inlines it (there `a` is an opaque pointer that every store may change), and
// the register allocation of the whole kernel, k-loop included, then comes out
// different.  Expanded in place the kernels compile to the instructions they had
// with private copies (profiles/conv_device_isa.txt).
#define LD_C8_EPILOGUE(ROW_FIRST, COL_FIRST, RAWC8)                                      \
  do {                                                                                   \
    const bool has_res = a.residual != nullptr;                                          \
    const bool res8 = a.res_c8 != nullptr; /* residual as a C8 image */                  \
    const bool has_y = a.y != nullptr;     /* fp32 output optional (C8-only nets) */     \
    const bool c8out = a.y_c8 != nullptr;                                                \
    const bool relu = a.relu != 0;                                                       \
    const bool has_aff = a.scale != nullptr, has_bias = a.bias != nullptr;               \
    size_t colbase[TN], c8base[TN];                                                      \
    bool jok[TN];                                                                        \
    const int prow = MODE == 1 ? a.Pfull : a.Pout;                                       \
    const rsrc_t r_sc = make_rsrc(a.scale, has_aff ? (unsigned)Cout * 4u : 0u);          \
    const rsrc_t r_sh = make_rsrc(a.shift, has_aff ? (unsigned)Cout * 4u : 0u);          \
    const rsrc_t r_bi = make_rsrc(a.bias, has_bias ? (unsigned)Cout * 4u : 0u);          \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                     \
      const int jc = (COL_FIRST) + j * 32 + l31;                                         \
      jok[j] = jc < a.J;                                                                 \
      const int n = jc / a.Pout;                                                         \
      int p = jc - n * a.Pout;                                                           \
      c8base[j] = ((size_t)n * (Cout >> 3) * a.Pout + p) * 16;                           \
      if (MODE == 1 && jok[j]) { /* compact class position -> full output position */    \
        int l, hc, wc;                                                                   \
        locate_out(a.g, p, l, hc, wc);                                                   \
        p = a.foff[l] + (2 * hc + a.ph) * a.fW[l] + 2 * wc + a.pw;                       \
      }                                                                                  \
      colbase[j] = (size_t)n * Cout * prow + p;                                          \
    }                                                                                    \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                     \
      const int rbase = (ROW_FIRST) + i * 32 + 4 * lk;                                   \
      _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                    \
        const int row0 = rbase + 8 * g; /* this lane's four rows: row0 .. row0 + 3 */    \
        const size_t c8row = (size_t)(row0 >> 3) * a.Pout * 16 + (row0 & 4) * 2;         \
        float sc[4], sh[4], bi[4], rv[TN][4];                                            \
        uintx2 rraw[TN];                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                               \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                  \
          const unsigned ro = (unsigned)(row0 + e) * 4u; /* >= Cout / absent: zeros */   \
          sc[e] = buf_load(r_sc, ro, 0);                                                 \
          sh[e] = buf_load(r_sh, ro, 0);                                                 \
          bi[e] = buf_load(r_bi, ro, 0);                                                 \
        }                                                                                \
        if (has_res) {                                                                   \
          _Pragma("unroll") for (int j = 0; j < TN; ++j)                                 \
          _Pragma("unroll") for (int e = 0; e < 4; ++e)                                  \
            rv[j][e] = (jok[j] && row0 + e < Cout)                                       \
                           ? a.residual[colbase[j] + (size_t)(row0 + e) * prow]          \
                           : 0.0f;                                                       \
        }                                                                                \
        if (MODE == 0 && res8) {                                                         \
          _Pragma("unroll") for (int j = 0; j < TN; ++j)                                 \
            rraw[j] = (jok[j] && row0 < Cout)                                            \
                          ? *(const uintx2*)((const char*)a.res_c8 + c8base[j] + c8row)  \
                          : uintx2{0u, 0u};                                              \
        }                                                                                \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                 \
          if (!jok[j]) continue;                                                         \
          floatx4_t q;                                                                   \
          floatx4_t rq = {0.0f, 0.0f, 0.0f, 0.0f};                                       \
          if (MODE == 0 && res8)                                                         \
            rq = __builtin_convertvector(__builtin_bit_cast(bf16x4, rraw[j]), floatx4_t); \
          _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                \
            const int r = 4 * g + e;                                                     \
            const int row = row0 + e;                                                    \
            float v = 0.0f;                                                              \
            if (row < Cout) {                                                            \
              v = acc[i][j][r] * (has_aff ? sc[e] : 1.0f) + (sh[e] + bi[e]);             \
              if (MODE == 0 && a.y_raw)                                                  \
                a.y_raw[colbase[j] + (size_t)row * prow] = acc[i][j][r];                 \
              if (has_res) v += rv[j][e];                                                \
              if (MODE == 0 && res8) v += rq[e];                                         \
              if (relu) v = fmaxf(v, 0.0f);                                              \
              if (has_y) a.y[colbase[j] + (size_t)row * prow] = v;                       \
            }                                                                            \
            q[e] = v;                                                                    \
          }                                                                              \
          if (MODE == 0 && c8out && row0 < Cout)                                         \
            *(uintx2*)((char*)a.y_c8 + c8base[j] + c8row) =                              \
                __builtin_bit_cast(uintx2, __builtin_convertvector(q, bf16x4));          \
          if ((RAWC8) && MODE == 0 && a.raw_c8 && row0 < Cout) {                         \
            const floatx4_t rw = {acc[i][j][4 * g], acc[i][j][4 * g + 1],                \
                                  acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};           \
            *(uintx2*)((char*)a.raw_c8 + c8base[j] + c8row) =                            \
                __builtin_bit_cast(uintx2, __builtin_convertvector(rw, bf16x4));         \
          }                                                                              \
        }                                                                                \
      }                                                                                  \
    }                                                                                    \
  } while (0)

