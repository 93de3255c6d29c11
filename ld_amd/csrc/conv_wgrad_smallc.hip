// Weight gradient of a small-Cin convolution (the 3 -> 64 7 x 7 ResNet stem, the
// 3 -> 32 3 x 3 first conv of the Res2Net deep stem): the backward counterpart of
// ld_conv_forward_smallc.
//
//   dW[co][r] = sum_j dY[co][j] * Xcol[r][j],  r = (ci, kh, kw) flat,  j = (n, ho, wo)
//
// The generic weight gradient gives every TAP a 128 (co) x 128 (ci) tile: 49 x 128 x
// 128 MACs per output position for the stem, of which 64 x 147 are useful.  Here the
// whole reduction index r is ONE GEMM dimension, padded to a multiple of 32 (the
// forward's flat form): Cout / 32 x ceil(R / 32) MFMA tiles (2 x 5 for the stem) per
// pair of output positions on v_mfma_f32_32x32x2f32.
//
// A workgroup (four waves) walks a contiguous range of tiles of 4 output rows x 32
// output columns of one image -- its SLAB of the reduction over j.  Per tile it
// stages the dY tile ([Cout][4 x 32], coalesced along wo) and the input patch
// ([Cin][3 S + KH][31 S + KW], every input pixel is read once and feeds up to KH KW /
// S^2 taps) in LDS; wave w then reduces over the 32 positions of output row w with
// ALL Cout x Rpad accumulators in registers (160 for the stem), reading the dY
// operand as [co = lane][j] and the patch operand as [r = lane][j] with a per-lane
// (ci, kh, kw) offset that is computed once.  At the end of the slab the four waves'
// accumulators are added in wave order through LDS and the workgroup writes ONE
// partial, laid out like dW.  The slabs are summed in slab order by the reduce launch
// the other weight gradients use (ld_wgrad_reduce_batch / the per-layer reduce): a
// slab IS the flat (Cout, Cin, KH, KW) array, described to them as one tap of a 1 x
// (Cout R) weight -- Cout R is a multiple of 4, so they take their 16-byte form,
// eight slab loads in flight, whatever R is.  No atomics; the slab count and every
// order are functions of the geometry: runs are bit-identical.
//
// Bound by: the MFMA pipes for the stem (10 MFMAs against 7 LDS reads per k pair;
// dY, 137 MB at 2 x 3 x 800 x 1344, is read once); by the dY read for Cout = 32 /
// R <= 32 (one MFMA per k pair).  Staging of a tile is not overlapped with ITS
// compute -- two resident workgroups per CU overlap each other's.
//
// x values that no valid output position reads still enter the patch (they meet a
// zero dY): non-finite inputs are outside the contract, as everywhere.
#include "conv_common.h"

namespace {

constexpr int kSTH = 4;                   // output rows per tile = waves per workgroup
constexpr int kSTW = 32;                  // output columns per tile
constexpr int kSYP = kSTH * kSTW + 1;     // dY tile row pitch (odd: conflict-free [co][j])
constexpr int kSMaxSlabs = 512;           // two workgroups per CU
constexpr int kSMaxR = 160;
constexpr int kSMaxLds = 72 * 1024;       // covers every geometry of the contract

struct SmallcWK {
  const float* x;   // (N, Cin, Hin * Win)
  const float* dy;  // (N, Cout, Hout * Wout)
  float* slabs;     // [slab][Cout][R]
  int Cin, KH, KW, stride, pad, Hin, Win, Hout, Wout;
  int R;                                // Cin * KH * KW
  int tiles_w, tiles_h, ntiles, chunk;  // chunk: tiles per slab
  int PR, PC, PCP;                      // patch rows / columns / row pitch
};

template <int MT, int NR>
__global__ __launch_bounds__(256, 2) void conv_wgrad_smallc_kernel(SmallcWK a) {
  constexpr int COUT = MT * 32, RPAD = NR * 32;
  extern __shared__ float lds[];
  float* ysm = lds;                // [COUT][kSYP]
  float* psm = lds + COUT * kSYP;  // [Cin][PR][PCP]
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int l31 = lane & 31, lk = lane >> 5;
  const int S = a.stride, PR = a.PR, PC = a.PC, PCP = a.PCP;
  const int Pin = a.Hin * a.Win, Pout = a.Hout * a.Wout;
  // (uniform) every (n, co, ho, wo0) row segment of dY starts on 16 bytes
  const bool dy_vec = a.Wout % 4 == 0 && ((uintptr_t)a.dy & 15) == 0;

  // this lane's patch offset of r = nr * 32 + l31 (rows r >= R: any valid cell,
  // their columns of the accumulators are never stored)
  int boff[NR];
#pragma unroll
  for (int nr = 0; nr < NR; ++nr) {
    const int r = nr * 32 + l31;
    const int ci = r / (a.KH * a.KW), rem = r - ci * (a.KH * a.KW);
    const int kh = rem / a.KW, kw = rem - kh * a.KW;
    boff[nr] = r < a.R ? (ci * PR + kh) * PCP + kw : 0;
  }
  floatx16 acc[MT][NR];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int tile0 = blockIdx.x * a.chunk;
  const int tile1 = min(a.ntiles, tile0 + a.chunk);
  for (int tile = tile0; tile < tile1; ++tile) {
    const int tw = tile % a.tiles_w;
    const int q = tile / a.tiles_w;
    const int th = q % a.tiles_h, n = q / a.tiles_h;
    const int ho0 = th * kSTH, wo0 = tw * kSTW;
    __syncthreads();  // the previous tile's operand reads are done
    {
      // the patch: four independent loads of a thread in flight per round
      const float* xn = a.x + (size_t)n * a.Cin * Pin;
      const int h00 = ho0 * S - a.pad, w00 = wo0 * S - a.pad;
      const int tot = a.Cin * PR * PC;
      for (int e0 = t; e0 < tot; e0 += 4 * 256) {
        float v[4];
        int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = e0 + u * 256;
          const int c = e % PC, qq = e / PC;
          const int r = qq % PR, ci = qq / PR;
          const int hi = h00 + r, wi = w00 + c;
          dst[u] = e < tot ? (ci * PR + r) * PCP + c : -1;
          v[u] = 0.0f;
          if (e < tot && hi >= 0 && hi < a.Hin && wi >= 0 && wi < a.Win)
            v[u] = xn[(size_t)ci * Pin + hi * a.Win + wi];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (dst[u] >= 0) psm[dst[u]] = v[u];
      }
      // the dY tile: 16-byte loads where every row segment is aligned
      const float* dyn = a.dy + (size_t)n * COUT * Pout;
      if (dy_vec) {
#pragma unroll 4
        for (int i = 0; i < COUT * kSTH * kSTW / 4 / 256; ++i) {
          const int e = t + i * 256;
          const int q4 = e & (kSTW / 4 - 1), hh = (e / (kSTW / 4)) & (kSTH - 1);
          const int co = e / (kSTH * kSTW / 4);
          const int ho = ho0 + hh, wo = wo0 + 4 * q4;
          float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (ho < a.Hout && wo < a.Wout)  // Wout % 4 == 0: all four or none
            v = *reinterpret_cast<const float4*>(dyn + (size_t)co * Pout + ho * a.Wout + wo);
          float* d = ysm + co * kSYP + hh * kSTW + 4 * q4;  // (odd pitch: four stores)
          d[0] = v.x;
          d[1] = v.y;
          d[2] = v.z;
          d[3] = v.w;
        }
      } else {
#pragma unroll 8
        for (int i = 0; i < COUT * kSTH * kSTW / 256; ++i) {
          const int e = t + i * 256;
          const int ww = e & (kSTW - 1), hh = (e / kSTW) & (kSTH - 1);
          const int co = e / (kSTH * kSTW);
          const int ho = ho0 + hh, wo = wo0 + ww;
          float v = 0.0f;
          if (ho < a.Hout && wo < a.Wout) v = dyn[(size_t)co * Pout + ho * a.Wout + wo];
          ysm[co * kSYP + hh * kSTW + ww] = v;
        }
      }
    }
    __syncthreads();
    if (ho0 + wave >= a.Hout) continue;  // (wave-uniform) a row of zeros
    // k pairs that hold a valid column (wave-uniform)
    const int npair = min(kSTW / 2, (a.Wout - wo0 + 1) / 2);
    const float* ap = ysm + l31 * kSYP + wave * kSTW + lk;
    const float* bp = psm + (wave * S) * PCP + lk * S;
    for (int kp = 0; kp < npair; ++kp) {
      float ra[MT], rb[NR];
#pragma unroll
      for (int i = 0; i < MT; ++i) ra[i] = ap[i * 32 * kSYP + 2 * kp];
#pragma unroll
      for (int j = 0; j < NR; ++j) rb[j] = bp[boff[j] + 2 * kp * S];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[i], rb[j], acc[i][j], 0, 0, 0);
    }
  }

  // the four waves' partials, added in wave order: red[co][RPAD] over the operands
  float* red = lds;
  for (int w = 0; w < kSTH; ++w) {
    __syncthreads();
    if (wave != w) continue;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          float* p = red + co * RPAD + j * 32 + l31;
          *p = w == 0 ? acc[i][j][r] : *p + acc[i][j][r];
        }
  }
  __syncthreads();
  float* slab = a.slabs + (size_t)blockIdx.x * COUT * a.R;
  for (int e = t; e < COUT * a.R; e += 256) {
    const int co = e / a.R, r = e - co * a.R;
    slab[e] = red[co * RPAD + r];
  }
}

struct SmallcPlan {
  SmallcWK k;
  int nslabs, mt, nr;
  size_t lds_bytes;
};

int smallc_plan(const ld_conv_t* c, SmallcPlan* p) {
  if (!c || c->N < 1 || c->Cin < 1 || c->Cout < 1 || c->KH < 1 || c->KW < 1 ||
      c->num_levels < 1 || c->num_levels > LD_MAX_LEVELS || c->pad < 0)
    return LD_EINVAL;
  const ld_conv_level_t& v = c->lv[0];
  if (c->num_levels != 1 || c->Cin >= 16 || (c->Cout != 32 && c->Cout != 64) ||
      c->Cin * c->KH * c->KW > kSMaxR || (c->stride != 1 && c->stride != 2))
    return LD_EUNSUPPORTED;
  if (v.Hin < 1 || v.Win < 1 || v.Hin + 2 * c->pad < c->KH || v.Win + 2 * c->pad < c->KW ||
      (v.Hin + 2 * c->pad - c->KH) / c->stride + 1 != v.Hout ||
      (v.Win + 2 * c->pad - c->KW) / c->stride + 1 != v.Wout || v.off_in != 0 ||
      v.off_out != 0 || (long long)v.Hin * v.Win != c->Pin ||
      (long long)v.Hout * v.Wout != c->Pout)
    return LD_EINVAL;
  SmallcWK& k = p->k;
  k.x = nullptr; k.dy = nullptr; k.slabs = nullptr;
  k.Cin = c->Cin; k.KH = c->KH; k.KW = c->KW; k.stride = c->stride; k.pad = c->pad;
  k.Hin = v.Hin; k.Win = v.Win; k.Hout = v.Hout; k.Wout = v.Wout;
  k.R = c->Cin * c->KH * c->KW;
  k.tiles_w = (v.Wout + kSTW - 1) / kSTW;
  k.tiles_h = (v.Hout + kSTH - 1) / kSTH;
  const long long nt = (long long)c->N * k.tiles_w * k.tiles_h;
  if (nt >= (1LL << 30)) return LD_EUNSUPPORTED;
  k.ntiles = (int)nt;
  k.chunk = (k.ntiles + kSMaxSlabs - 1) / kSMaxSlabs;
  p->nslabs = (k.ntiles + k.chunk - 1) / k.chunk;
  k.PR = (kSTH - 1) * c->stride + c->KH;
  k.PC = (kSTW - 1) * c->stride + c->KW;
  k.PCP = k.PC | 1;
  p->mt = c->Cout / 32;
  p->nr = (k.R + 31) / 32;
  const size_t stage = (size_t)c->Cout * kSYP + (size_t)c->Cin * k.PR * k.PCP;
  const size_t red = (size_t)c->Cout * p->nr * 32;
  p->lds_bytes = (stage > red ? stage : red) * sizeof(float);
  if (p->lds_bytes > (size_t)kSMaxLds) return LD_EUNSUPPORTED;
  return 0;
}

template <int MT, int NR>
int smallc_launch_one(const SmallcPlan& p, hipStream_t stream) {
  auto kern = conv_wgrad_smallc_kernel<MT, NR>;
  static const hipError_t attr = hipFuncSetAttribute(
      (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kSMaxLds);
  if (attr != hipSuccess) return (int)attr;
  LD_LAUNCH(kern, dim3(p.nslabs), dim3(256), p.lds_bytes, stream, p.k);
  return (int)hipGetLastError();
}

template <int MT>
int smallc_launch_mt(const SmallcPlan& p, hipStream_t stream) {
  switch (p.nr) {
    case 1: return smallc_launch_one<MT, 1>(p, stream);
    case 2: return smallc_launch_one<MT, 2>(p, stream);
    case 3: return smallc_launch_one<MT, 3>(p, stream);
    case 4: return smallc_launch_one<MT, 4>(p, stream);
    case 5: return smallc_launch_one<MT, 5>(p, stream);
  }
  return LD_EUNSUPPORTED;
}

// the slabs of one weight gradient into `workspace`; *nslabs / *R for the reduce
int smallc_partials(const ld_conv_t* c, const float* x, const float* dy, void* workspace,
                    size_t workspace_bytes, hipStream_t stream, int* nslabs, int* R) {
  SmallcPlan p;
  if (int e = smallc_plan(c, &p)) return e;
  if (!x || !dy || !workspace) return LD_EINVAL;
  if (workspace_bytes < (size_t)p.nslabs * c->Cout * p.k.R * sizeof(float)) return LD_ENOSPACE;
  p.k.x = x;
  p.k.dy = dy;
  p.k.slabs = (float*)workspace;
  *nslabs = p.nslabs;
  *R = p.k.R;
  return p.mt == 1 ? smallc_launch_mt<1>(p, stream) : smallc_launch_mt<2>(p, stream);
}

}  // namespace

extern "C" int ld_conv_wgrad_smallc_supported(const ld_conv_t* c) {
  SmallcPlan p;
  return smallc_plan(c, &p) == 0 ? 1 : 0;
}

extern "C" int ld_conv_wgrad_smallc_slabs(const ld_conv_t* c) {
  SmallcPlan p;
  if (int e = smallc_plan(c, &p)) return e;
  return p.nslabs;
}

extern "C" size_t ld_conv_wgrad_smallc_workspace_bytes(const ld_conv_t* c) {
  SmallcPlan p;
  if (smallc_plan(c, &p)) return 0;
  return (size_t)p.nslabs * c->Cout * p.k.R * sizeof(float);
}

extern "C" int ld_conv_wgrad_smallc(const ld_conv_t* c, const float* x, const float* dy,
                                    float* dw, int accumulate, void* workspace,
                                    size_t workspace_bytes, ld_stream_t stream) {
  if (!dw) return LD_EINVAL;
  int nslabs = 0, R = 0;
  if (int e = smallc_partials(c, x, dy, workspace, workspace_bytes, (hipStream_t)stream,
                              &nslabs, &R))
    return e;
  return ld_wgrad_reduce_launch((const float*)workspace, nslabs, 1, 1, c->Cout * R, dw,
                                accumulate, (hipStream_t)stream);
}

extern "C" int ld_conv_wgrad_smallc_partial(const ld_conv_t* c, const float* x,
                                            const float* dy, void* slabs, size_t slab_bytes,
                                            ld_wgrad_job_t* job, ld_stream_t stream) {
  if (!job) return LD_EINVAL;
  int nslabs = 0, R = 0;
  if (int e = smallc_partials(c, x, dy, slabs, slab_bytes, (hipStream_t)stream, &nslabs, &R))
    return e;
  job->slabs = (const float*)slabs;
  job->splits = nslabs;
  job->ntaps = 1;
  job->Cout = 1;  // the flat dW (see the head of this file)
  job->Cin = c->Cout * R;
  return 0;
}
