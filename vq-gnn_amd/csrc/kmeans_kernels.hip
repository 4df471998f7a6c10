// Device k-means++ codebook initialisation for all nb branches of a layer
// (include/vqgnn.h §12).  Replaces the per-branch CPU MiniBatchKMeans fits of
// vq_gnn_v1/models.py:147-159, whose centroids feed
// VectorQuantizerEMA.feature_kmeans_init (vq_gnn_v2/vq.py:102-105).
//
// Points.  Branch b's points are the normalised rows z = fma(x - shift, alpha,
// beta) of columns D*b .. D*b + W - 1 -- the assign's expression on the
// assign's coefficient table -- written once, branch-major [nb][B][W], into
// the workspace (a branch's rows in X are W*4-byte slices at a row stride:
// every later step would read them uncoalesced).
//
// Distance (the assign's reference arithmetic): zz and cc are
// sequential fp32 sums of squares in k order (separate multiply and add),
// dot = z0 c0 then a k-ordered fmaf chain, d = fmaf(-2, dot, zz + cc).
//
// Seeding = k-means++ with one trial per step, reproducible bit for bit
// (tests/kmeans_ref.py restates it):
//   r(b, s) = mix(mix(seed ^ mix(b)) + s), mix = the random walk's splitmix64
//   step 0 picks row r(b, 0) mod B.  After picking row i* at step s:
//     centroid[b][s] = z[i*]
//     mind[i] = min(mind[i], max(d(z_i, c_s), 0)) for every row (mind = +inf
//     at the start), then mind[i*] = 0 exactly
//   weight of row i: q_i = llrint(min(mind_i, 2^20) * 2^20) -- exact (a power
//   of two times a 24-bit significand, <= 2^40), so the sum over B <= 2^23
//   rows is an exact integer whatever the reduction tree
//   step s >= 1: T = sum q_i; T = 0 -> row r(b, s) mod B; else t = r(b, s)
//   mod T and the first row whose inclusive prefix sum exceeds t.
// Two launches per step over kKmPart-row parts: kmeans_mind_kernel (grid
// (parts, nb)) folds the newest centroid into mind and writes each part's
// sum; kmeans_pick_kernel (one workgroup per branch) scans the part sums for
// the part, that part's q for the row, and writes seed_rows[b][s] and the
// centroid.  No host synchronisation, no readback, no atomics: 2 M launches
// after the staging launch.
//
// Lloyd step = vqgnn_vq_assign (labels, per-codeword counts and fixed-point
// sums in one launch) + kmeans_centroid_kernel: c_k = (float)((double)S_k *
// 2^-shift / (double)n) for n > 0, the centroid kept for n = 0.
//
// Dead-codeword revival (include/vqgnn.h §13, tests/revive_ref.py) runs the
// same D^2 step against the live codebook: mind starts from the assign's
// labels instead of +inf, and the row picked at step s becomes the s-th dead
// codeword of its branch.  km_fold_part and km_pick_row are the step both use.
// 1 + 2R launches: revive_stage_kernel (points + slots), revive_mind_kernel,
// then revive_pick_kernel / revive_fold_kernel per step.
#include "common.h"

namespace vqgnn {

namespace {

using u64 = unsigned long long;

constexpr int kKmThreads = 256;
constexpr int kKmWaves = kKmThreads / 64;
constexpr int kKmRows = 4;                      // rows per thread and part
constexpr int kKmPart = kKmThreads * kKmRows;   // rows per part
constexpr int kKmMaxW = 8;

// the random walk's splitmix64 finaliser (subgraph_kernels.hip, walk_mix)
__device__ __forceinline__ u64 km_mix(u64 z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ u64 km_draw(u64 seed, int b, int s) {
  return km_mix(km_mix(seed ^ km_mix((u64)b)) + (u64)s);
}

// q = llrint(min(mind, 2^20) * 2^20): the product is exact, rintf rounds to
// nearest-even, the result is an integer <= 2^40
__device__ __forceinline__ u64 km_weight(float m) {
  return (u64)rintf(__fmul_rn(fminf(m, 1048576.f), 1048576.f));
}

__device__ __forceinline__ float km_sumsq(const float (&v)[kKmMaxW], int W) {
  float s = __fmul_rn(v[0], v[0]);
#pragma unroll
  for (int k = 1; k < kKmMaxW; ++k)
    if (k < W) s = __fadd_rn(s, __fmul_rn(v[k], v[k]));
  return s;
}

__device__ __forceinline__ float km_dist(const float (&z)[kKmMaxW], const float (&c)[kKmMaxW],
                                         float cc, int W) {
  const float zz = km_sumsq(z, W);
  float dot = __fmul_rn(z[0], c[0]);
#pragma unroll
  for (int k = 1; k < kKmMaxW; ++k)
    if (k < W) dot = fmaf(z[k], c[k], dot);
  return fmaf(-2.f, dot, __fadd_rn(zz, cc));
}

// Inclusive scan of one u64 per thread over the workgroup (wave scan through
// __shfl_up, wave totals through LDS); *total = the workgroup's sum.  Safe to
// call repeatedly on the same wsum.
__device__ __forceinline__ u64 km_block_scan(u64 v, u64* wsum, u64* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();                 // the previous call's readers are done
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  u64 base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kKmWaves; ++w) {
    const u64 s = wsum[w];
    if (w < wave) base += s;
    tot += s;
  }
  *total = tot;
  return x + base;
}

// Z[b][i][k] = fma(x - shift, alpha, beta); mind[b][i] = +inf.  One thread
// per (row, branch), branch fastest: a wave reads consecutive slices of a row.
__global__ void __launch_bounds__(kKmThreads)
kmeans_stage_kernel(const float* __restrict__ X, int64_t ldx, int B, int nb, int D, int W,
                    const float* __restrict__ coef, float* __restrict__ Z,
                    float* __restrict__ mind) {
  const int64_t g = (int64_t)blockIdx.x * kKmThreads + threadIdx.x;
  if (g >= (int64_t)B * nb) return;
  const int i = (int)(g / nb), b = (int)(g % nb);
  const int F = nb * D;
  const float* x = X + (int64_t)i * ldx + (int64_t)b * D;
  float* z = Z + ((int64_t)b * B + i) * W;
#pragma clang loop vectorize(disable) interleave(disable)
  for (int k = 0; k < W; ++k) {
    const int c = b * D + k;
    z[k] = fmaf(__fsub_rn(x[k], coef[4 * F + c]), coef[c], coef[F + c]);
  }
  mind[(int64_t)b * B + i] = __builtin_inff();
}

__device__ __forceinline__ void km_load_row(const float* __restrict__ p, int W,
                                            float (&v)[kKmMaxW]) {
  if (W == 4) {       // 16-byte rows of a 256-byte aligned array
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
#pragma unroll
    for (int k = 4; k < kKmMaxW; ++k) v[k] = 0.f;
    return;
  }
#pragma unroll
  for (int k = 0; k < kKmMaxW; ++k) v[k] = k < W ? p[k] : 0.f;
}

// One part of the D^2 step's fold: mind[i] = min(mind[i], max(d(z_i, c), 0))
// over the part's rows, mind[istar] = 0 exactly; thread 0 writes the part's
// sum of q.  Shared by the seeding and the revival (§13).
__device__ __forceinline__ void km_fold_part(const float* __restrict__ zb, float* __restrict__ mb,
                                             const float (&c)[kKmMaxW], int istar, int part, int B,
                                             int W, u64* __restrict__ partial) {
  __shared__ u64 wsum[kKmWaves];
  const int tid = threadIdx.x;
  const float cc = km_sumsq(c, W);
  u64 sum = 0;
#pragma unroll
  for (int j = 0; j < kKmRows; ++j) {
    const int i = part * kKmPart + j * kKmThreads + tid;
    if (i < B) {
      float z[kKmMaxW];
      km_load_row(zb + (int64_t)i * W, W, z);
      float m = fminf(mb[i], fmaxf(km_dist(z, c, cc, W), 0.f));
      if (i == istar) m = 0.f;
      mb[i] = m;
      sum += km_weight(m);
    }
  }
  u64 total;
  km_block_scan(sum, wsum, &total);
  if (tid == 0) *partial = total;
}

// The D^2 draw of one branch by its workgroup: T = the sum of the part sums
// pb[0 .. P) when `weighted`; T = 0 (or not weighted: the seeding's step 0)
// -> row r mod B, else t = r mod T and the first row whose inclusive prefix
// sum of q exceeds t.  The same row in every thread.  Shared by the seeding
// and the revival (§13).
__device__ __forceinline__ int km_pick_row(const u64* __restrict__ pb, int P,
                                           const float* __restrict__ mb, int B, u64 r,
                                           bool weighted) {
  __shared__ u64 wsum[kKmWaves];
  __shared__ u64 sh_t;
  __shared__ int sh_part, sh_row;
  const int tid = threadIdx.x;
  if (tid == 0) sh_part = -1, sh_row = -1;
  u64 T = 0;
  if (weighted) {
    u64 acc = 0;
    for (int p = tid; p < P; p += kKmThreads) acc += pb[p];
    km_block_scan(acc, wsum, &T);
  }
  int row = (int)(r % (u64)B);          // step 0, and T = 0 (every row is a seed's copy)
  if (T != 0) {                         // uniform over the workgroup
    const u64 t = r % T;
    u64 carry = 0;
    for (int p0 = 0; p0 < P; p0 += kKmThreads) {
      const int p = p0 + tid;
      const u64 v = p < P ? pb[p] : 0;
      u64 tot;
      const u64 incl = km_block_scan(v, wsum, &tot) + carry;
      const u64 excl = incl - v;
      if (excl <= t && t < incl) sh_part = p, sh_t = t - excl;
      carry += tot;
    }
    __syncthreads();
    const int part = sh_part;
    if (part >= 0) {                    // always: the part sums add up to T
      const u64 tr = sh_t;
      const int i0 = part * kKmPart + tid * kKmRows;
      u64 q[kKmRows], sum = 0;
#pragma unroll
      for (int j = 0; j < kKmRows; ++j) {
        q[j] = i0 + j < B ? km_weight(mb[i0 + j]) : 0;
        sum += q[j];
      }
      u64 tot;
      u64 excl = km_block_scan(sum, wsum, &tot) - sum;
#pragma unroll
      for (int j = 0; j < kKmRows; ++j) {
        if (excl <= tr && tr < excl + q[j]) sh_row = i0 + j;
        excl += q[j];
      }
      __syncthreads();
      if (sh_row >= 0 && sh_row < B) row = sh_row;
    }
  }
  return row;
}

// Fold centroid s (row seed_rows[b][s]) into mind; partials[b][part] = the
// part's sum of q.
__global__ void __launch_bounds__(kKmThreads)
kmeans_mind_kernel(const float* __restrict__ Z, float* __restrict__ mind,
                   const float* __restrict__ cent, int ldw, int64_t cen_bstride,
                   const int* __restrict__ seed_rows, int M, int s, int B, int W,
                   u64* __restrict__ partials, int P) {
  const int part = blockIdx.x, b = blockIdx.y;
  float c[kKmMaxW];
  const float* cp = cent + (int64_t)b * cen_bstride + (int64_t)s * ldw;
#pragma unroll
  for (int k = 0; k < kKmMaxW; ++k) c[k] = k < W ? cp[k] : 0.f;
  km_fold_part(Z + (int64_t)b * B * W, mind + (int64_t)b * B, c, seed_rows[(int64_t)b * M + s],
               part, B, W, partials + (int64_t)b * P + part);
}

// Step s of branch b = blockIdx.x: the D^2 draw over the part sums and the
// chosen part's rows; writes seed_rows[b][s] and centroid[b][s].
__global__ void __launch_bounds__(kKmThreads)
kmeans_pick_kernel(const float* __restrict__ Z, const float* __restrict__ mind,
                   const u64* __restrict__ partials, int P, int B, int W, int M, int s, u64 seed,
                   float* __restrict__ cent, int ldw, int64_t cen_bstride,
                   int* __restrict__ seed_rows) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int row = km_pick_row(partials + (int64_t)b * P, P, mind + (int64_t)b * B, B,
                              km_draw(seed, b, s), s > 0);
  if (tid == 0) seed_rows[(int64_t)b * M + s] = row;
  if (tid < W)
    cent[(int64_t)b * cen_bstride + (int64_t)s * ldw + tid] = Z[((int64_t)b * B + row) * W + tid];
}

// Centroid update from the assign's statistic slab(s) [nparts][nb][M][W+1]
// (count, fixed-point sums): one thread per codeword.  update = 0: counts and
// the empty-cluster count only.  Clears what it reads.
__global__ void __launch_bounds__(kKmThreads)
kmeans_centroid_kernel(long long* __restrict__ stats, int nparts, int64_t part_stride, int shift,
                       int nb, int M, int W, float* __restrict__ cent, int ldw,
                       int64_t cen_bstride, int update, long long* __restrict__ counts,
                       int* __restrict__ n_empty) {
  const int64_t g = (int64_t)blockIdx.x * kKmThreads + threadIdx.x;
  const bool live = g < (int64_t)nb * M;
  int empty = 0;
  if (live) {
    const int b = (int)(g / M), m = (int)(g % M);
    long long* st = stats + g * (W + 1);
    auto stat = [&](int k) {
      long long v = 0;
      for (int p = 0; p < nparts; ++p) {
        v += st[(int64_t)p * part_stride + k];
        st[(int64_t)p * part_stride + k] = 0;
      }
      return v;
    };
    const long long n = stat(0);
    float* c = cent + (int64_t)b * cen_bstride + (int64_t)m * ldw;
    for (int k = 0; k < W; ++k) {
      const long long S = stat(1 + k);
      if (update && n > 0) c[k] = (float)(ldexp((double)S, -shift) / (double)n);
    }
    if (counts) counts[g] = n;
    empty = n == 0;
  }
  const int block_empty = __syncthreads_count(empty);
  if (n_empty && threadIdx.x == 0 && block_empty) atomicAdd(n_empty, block_empty);
}

struct KmWs {
  float* Z;
  float* mind;
  u64* partials;
  int P;
  size_t bytes;
};

KmWs km_ws(void* workspace, int B, int nb, int W) {
  KmWs w;
  w.P = (B + kKmPart - 1) / kKmPart;
  char* p = static_cast<char*>(workspace);
  size_t off = 0;
  w.Z = reinterpret_cast<float*>(p + off);
  off += align_up((size_t)nb * B * W * sizeof(float), 256);
  w.mind = reinterpret_cast<float*>(p + off);
  off += align_up((size_t)nb * B * sizeof(float), 256);
  w.partials = reinterpret_cast<u64*>(p + off);
  off += align_up((size_t)nb * w.P * sizeof(u64), 256);
  w.bytes = off;
  return w;
}

// ---- dead-codeword revival (include/vqgnn.h §13) ------------------------- //
// The codebook state a revival writes, and what it reads beside it.
struct Revive {
  float* cs;                 // [nb][M], branch stride cs_bstride
  int64_t cs_bstride;
  float* ema_w;              // ema_w / emb / emb_out [nb][M][ldw], one layout
  float* emb;
  float* emb_out;
  int ldw;
  int64_t emb_bstride;
  const float* rm_f;         // [nb][D] running statistics of the feature BatchNorm
  const float* rv_f;
  short* codes;              // optional scatter of the revived rows' codes
  int64_t ldc;
  const int64_t* batch_idx;
  int* n_slots;              // [nb]
  int* slots;                // [nb][R]
  int* rows;                 // [nb][R]
  int R;
  float threshold, init_count;
};

// Launch 1.  Blocks [0, cell_blocks): the staging of kmeans_stage_kernel
// without mind.  Blocks cell_blocks + b: branch b's slots -- the first R of
// the m with cs[b][m] < threshold in ascending m (an ordered compaction by
// block scans over 256-codeword chunks), n_slots[b], -1 in the unused slots
// and in every row entry (the picks overwrite the used ones).
__global__ void __launch_bounds__(kKmThreads)
revive_stage_kernel(const float* __restrict__ X, int64_t ldx, int B, int nb, int D, int M,
                    const float* __restrict__ coef, float* __restrict__ Z, unsigned cell_blocks,
                    Revive v) {
  if (blockIdx.x >= cell_blocks) {
    __shared__ u64 wsum[kKmWaves];
    const int b = blockIdx.x - cell_blocks, tid = threadIdx.x, R = v.R;
    const float* cs = v.cs + (int64_t)b * v.cs_bstride;
    int* slots = v.slots + (int64_t)b * R;
    u64 carry = 0;
    for (int m0 = 0; m0 < M; m0 += kKmThreads) {
      const int m = m0 + tid;
      const u64 dead = m < M && cs[m] < v.threshold ? 1 : 0;   // a NaN is not dead
      u64 tot;
      const u64 pos = km_block_scan(dead, wsum, &tot) + carry - dead;
      if (dead && pos < (u64)R) slots[pos] = m;
      carry += tot;
    }
    const int n = carry < (u64)R ? (int)carry : R;
    if (tid == 0) v.n_slots[b] = n;
    for (int j = tid; j < R; j += kKmThreads) {
      if (j >= n) slots[j] = -1;
      v.rows[(int64_t)b * R + j] = -1;
    }
    return;
  }
  const int64_t g = (int64_t)blockIdx.x * kKmThreads + threadIdx.x;
  if (g >= (int64_t)B * nb) return;
  const int i = (int)(g / nb), b = (int)(g % nb);
  const int F = nb * D;
  const float* x = X + (int64_t)i * ldx + (int64_t)b * D;
  float* z = Z + ((int64_t)b * B + i) * D;
#pragma clang loop vectorize(disable) interleave(disable)
  for (int k = 0; k < D; ++k) {
    const int c = b * D + k;
    z[k] = fmaf(__fsub_rn(x[k], coef[4 * F + c]), coef[c], coef[F + c]);
  }
}

// Launch 2.  mind[b][i] = max(d(z_i, emb[b][labels[b][i]][:D]), 0), 0 for a
// label outside [0, M); partials[b][part] = the part's sum of q.
__global__ void __launch_bounds__(kKmThreads)
revive_mind_kernel(const float* __restrict__ Z, float* __restrict__ mind,
                   const int64_t* __restrict__ labels, const float* __restrict__ emb, int ldw,
                   int64_t emb_bstride, int M, int B, int D, u64* __restrict__ partials, int P) {
  __shared__ u64 wsum[kKmWaves];
  const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* zb = Z + (int64_t)b * B * D;
  const float* eb = emb + (int64_t)b * emb_bstride;
  const int64_t* lb = labels + (int64_t)b * B;
  float* mb = mind + (int64_t)b * B;
  u64 sum = 0;
#pragma unroll
  for (int j = 0; j < kKmRows; ++j) {
    const int i = part * kKmPart + j * kKmThreads + tid;
    if (i < B) {
      const int64_t lab = lb[i];
      float m = 0.f;
      if (lab >= 0 && lab < M) {
        float z[kKmMaxW], c[kKmMaxW];
        km_load_row(zb + (int64_t)i * D, D, z);
        const float* cp = eb + lab * ldw;
#pragma unroll
        for (int k = 0; k < kKmMaxW; ++k) c[k] = k < D ? cp[k] : 0.f;
        m = fmaxf(km_dist(z, c, km_sumsq(c, D), D), 0.f);
      }
      mb[i] = m;
      sum += km_weight(m);
    }
  }
  u64 total;
  km_block_scan(sum, wsum, &total);
  if (tid == 0) partials[(int64_t)b * P + part] = total;
}

// Step s of branch b = blockIdx.x, a no-op past n_slots[b] (slots[b][s] = -1
// there): the seeding's draw, then the picked row becomes codeword slots[b][s].
__global__ void __launch_bounds__(kKmThreads)
revive_pick_kernel(const float* __restrict__ Z, const float* __restrict__ mind,
                   const u64* __restrict__ partials, int P, int B, int D, int s, u64 seed,
                   Revive v) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int m = v.slots[(int64_t)b * v.R + s];
  if (m < 0) return;                             // s >= n_slots[b]; uniform over the workgroup
  const int row = km_pick_row(partials + (int64_t)b * P, P, mind + (int64_t)b * B, B,
                              km_draw(seed, b, s), true);
  if (tid == 0) {
    v.rows[(int64_t)b * v.R + s] = row;
    v.cs[(int64_t)b * v.cs_bstride + m] = v.init_count;
    if (v.codes) v.codes[v.batch_idx[row] * v.ldc + b] = (short)m;
  }
  if (tid < D) {
    const int64_t o = (int64_t)b * v.emb_bstride + (int64_t)m * v.ldw + tid;
    const float z = Z[((int64_t)b * B + row) * D + tid];
    v.emb[o] = z;
    v.ema_w[o] = __fmul_rn(z, v.init_count);
    // the finalize's feature half (ema_finalize.h): emb*sqrt(rv+1e-5)+rm
    const float sd = sqrtf(__fadd_rn(v.rv_f[b * D + tid], 1e-5f));
    v.emb_out[o] = __fadd_rn(__fmul_rn(z, sd), v.rm_f[b * D + tid]);
    // the gradient half stays where it is; ema_w follows the new cluster size
    if (v.ldw >= 2 * D) v.ema_w[o + D] = __fmul_rn(v.emb[o + D], v.init_count);
  }
}

// Fold the row picked at step s (z of rows[b][s]) into mind; a no-op past
// n_slots[b] (rows[b][s] = -1 there; the part sums then stay as they are, and
// nothing reads them).
__global__ void __launch_bounds__(kKmThreads)
revive_fold_kernel(const float* __restrict__ Z, float* __restrict__ mind,
                   const int* __restrict__ rows, int R, int s, int B, int D,
                   u64* __restrict__ partials, int P) {
  const int part = blockIdx.x, b = blockIdx.y;
  const int istar = rows[(int64_t)b * R + s];
  if (istar < 0) return;                         // s >= n_slots[b]; uniform over the workgroup
  const float* zb = Z + (int64_t)b * B * D;
  float c[kKmMaxW];
  km_load_row(zb + (int64_t)istar * D, D, c);
  km_fold_part(zb, mind + (int64_t)b * B, c, istar, part, B, D,
               partials + (int64_t)b * P + part);
}

bool revive_shape_ok(int B, int nb, int D, int M, int R) {
  return B > 0 && nb > 0 && D > 0 && D <= kKmMaxW && M > 0 && M <= B && B <= (1 << 23) &&
         M <= 32767 && R >= 1 && R <= M;
}

}  // namespace

}  // namespace vqgnn

using namespace vqgnn;

extern "C" size_t vqgnn_kmeans_workspace(int32_t B, int32_t nb, int32_t M, int32_t W) {
  if (B <= 0 || nb <= 0 || M <= 0 || W <= 0 || W > kKmMaxW) return 0;
  return km_ws(nullptr, B, nb, W).bytes;
}

extern "C" int vqgnn_kmeans_seed(const float* X, int64_t ldx, int32_t B, int32_t nb, int32_t D,
                                 int32_t M, int32_t W, const float* coef, uint64_t seed,
                                 float* centroids, int32_t ldw, int64_t cen_bstride,
                                 int32_t* seed_rows, void* workspace, vqgnn_stream_t stream) {
  clear_error();
  VQGNN_REQUIRE(X && coef && centroids && seed_rows && workspace, "kmeans_seed: null pointer");
  VQGNN_REQUIRE(B > 0 && nb > 0 && D > 0 && M > 0 && W > 0, "kmeans_seed: bad shape");
  VQGNN_REQUIRE(W <= kKmMaxW, "kmeans_seed: W=%d > 8 not implemented", W);
  VQGNN_REQUIRE(W <= D, "kmeans_seed: W=%d exceeds the branch width D=%d", W, D);
  VQGNN_REQUIRE(B <= (1 << 23), "kmeans_seed: B=%d rows exceed 2^23", B);
  VQGNN_REQUIRE(M <= B, "kmeans_seed: M=%d seeds from B=%d rows", M, B);
  VQGNN_REQUIRE(M <= 32767, "kmeans_seed: int16 codes need M <= 32767");
  VQGNN_REQUIRE(ldx >= (int64_t)nb * D, "kmeans_seed: ldx too small");
  VQGNN_REQUIRE((int64_t)B * ldx * 4 < ((int64_t)1 << 32), "kmeans_seed: B*ldx must span < 4 GiB");
  VQGNN_REQUIRE(ldw >= W && cen_bstride >= (int64_t)M * ldw, "kmeans_seed: bad centroid layout");
  hipStream_t st = as_stream(stream);
  const KmWs w = km_ws(workspace, B, nb, W);
  const int64_t cells = (int64_t)B * nb;
  hipLaunchKernelGGL(kmeans_stage_kernel, dim3((unsigned)((cells + kKmThreads - 1) / kKmThreads)),
                     dim3(kKmThreads), 0, st, X, ldx, B, nb, D, W, coef, w.Z, w.mind);
  for (int s = 0; s < M; ++s) {
    if (s > 0)
      hipLaunchKernelGGL(kmeans_mind_kernel, dim3(w.P, nb), dim3(kKmThreads), 0, st, w.Z, w.mind,
                         centroids, ldw, cen_bstride, seed_rows, M, s - 1, B, W, w.partials, w.P);
    hipLaunchKernelGGL(kmeans_pick_kernel, dim3(nb), dim3(kKmThreads), 0, st, w.Z, w.mind,
                       w.partials, w.P, B, W, M, s, (u64)seed, centroids, ldw, cen_bstride,
                       seed_rows);
  }
  return check_launch("kmeans_seed");
}

extern "C" int vqgnn_kmeans_centroids(int64_t* ema_parts, int32_t nparts, int64_t stat_count,
                                      int32_t nb, int32_t M, int32_t W, float* centroids,
                                      int32_t ldw, int64_t cen_bstride, int32_t update,
                                      int64_t* counts, int32_t* n_empty, vqgnn_stream_t stream) {
  clear_error();
  VQGNN_REQUIRE(ema_parts && (centroids || !update), "kmeans_centroids: null pointer");
  VQGNN_REQUIRE(nparts > 0 && nb > 0 && M > 0 && W > 0 && stat_count > 0,
                "kmeans_centroids: bad shape");
  VQGNN_REQUIRE(W <= kKmMaxW, "kmeans_centroids: W=%d > 8 not implemented", W);
  VQGNN_REQUIRE(!update || (ldw >= W && cen_bstride >= (int64_t)M * ldw),
                "kmeans_centroids: bad centroid layout");
  hipStream_t st = as_stream(stream);
  int32_t shift_f = 0;
  vqgnn_vq_stat_shifts(stat_count, 1.f, &shift_f, nullptr);
  if (n_empty && hipMemsetAsync(n_empty, 0, sizeof(int32_t), st) != hipSuccess)
    return check_launch("kmeans_centroids memset");
  const int64_t cells = (int64_t)nb * M;
  hipLaunchKernelGGL(kmeans_centroid_kernel,
                     dim3((unsigned)((cells + kKmThreads - 1) / kKmThreads)), dim3(kKmThreads), 0,
                     st, reinterpret_cast<long long*>(ema_parts), nparts, cells * (W + 1), shift_f,
                     nb, M, W, centroids, ldw, cen_bstride, update,
                     reinterpret_cast<long long*>(counts), n_empty);
  return check_launch("kmeans_centroids");
}

extern "C" size_t vqgnn_vq_revive_workspace(int32_t B, int32_t nb, int32_t D, int32_t M,
                                            int32_t max_revive) {
  if (!revive_shape_ok(B, nb, D, M, max_revive)) return 0;
  return km_ws(nullptr, B, nb, D).bytes;
}

extern "C" int vqgnn_vq_revive(const float* X, int64_t ldx, int32_t B, int32_t nb, int32_t D,
                               int32_t M, const float* coef, const int64_t* labels,
                               float threshold, int32_t max_revive, float init_count,
                               uint64_t seed, float* cluster_size, int64_t cs_bstride,
                               float* ema_w, float* embedding, float* embedding_output,
                               int32_t ldw, int64_t emb_bstride, const float* rm_f,
                               const float* rv_f, int16_t* codes, int64_t ldc,
                               const int64_t* batch_idx, int32_t* n_slots, int32_t* slots,
                               int32_t* rows, void* workspace, vqgnn_stream_t stream) {
  clear_error();
  VQGNN_REQUIRE(X && coef && labels && cluster_size && ema_w && embedding && embedding_output &&
                    rm_f && rv_f && n_slots && slots && rows && workspace,
                "vq_revive: null pointer");
  VQGNN_REQUIRE(B > 0 && nb > 0 && D > 0 && M > 0, "vq_revive: bad shape");
  VQGNN_REQUIRE(D <= kKmMaxW, "vq_revive: D=%d > 8 not implemented", D);
  VQGNN_REQUIRE(B <= (1 << 23), "vq_revive: B=%d rows exceed 2^23", B);
  VQGNN_REQUIRE(M <= B, "vq_revive: M=%d codewords from B=%d rows", M, B);
  VQGNN_REQUIRE(M <= 32767, "vq_revive: int16 codes need M <= 32767");
  VQGNN_REQUIRE(max_revive >= 1 && max_revive <= M, "vq_revive: max_revive=%d outside [1, M=%d]",
                max_revive, M);
  VQGNN_REQUIRE(ldx >= (int64_t)nb * D, "vq_revive: ldx too small");
  VQGNN_REQUIRE((int64_t)B * ldx * 4 < ((int64_t)1 << 32), "vq_revive: B*ldx must span < 4 GiB");
  VQGNN_REQUIRE((ldw == D || ldw >= 2 * D) && emb_bstride >= (int64_t)M * ldw && cs_bstride >= M,
                "vq_revive: bad codebook layout");
  VQGNN_REQUIRE(!(init_count < threshold), "vq_revive: init_count below the threshold");
  VQGNN_REQUIRE(!codes || (batch_idx && ldc >= nb), "vq_revive: codes needs batch_idx, ldc>=nb");
  hipStream_t st = as_stream(stream);
  const KmWs w = km_ws(workspace, B, nb, D);
  const int R = max_revive;
  Revive v;
  v.cs = cluster_size, v.cs_bstride = cs_bstride;
  v.ema_w = ema_w, v.emb = embedding, v.emb_out = embedding_output;
  v.ldw = ldw, v.emb_bstride = emb_bstride;
  v.rm_f = rm_f, v.rv_f = rv_f;
  v.codes = codes, v.ldc = ldc, v.batch_idx = batch_idx;
  v.n_slots = n_slots, v.slots = slots, v.rows = rows, v.R = R;
  v.threshold = threshold, v.init_count = init_count;
  const int64_t cells = (int64_t)B * nb;
  const unsigned cell_blocks = (unsigned)((cells + kKmThreads - 1) / kKmThreads);
  hipLaunchKernelGGL(revive_stage_kernel, dim3(cell_blocks + nb), dim3(kKmThreads), 0, st, X, ldx,
                     B, nb, D, M, coef, w.Z, cell_blocks, v);
  hipLaunchKernelGGL(revive_mind_kernel, dim3(w.P, nb), dim3(kKmThreads), 0, st, w.Z, w.mind,
                     labels, embedding, ldw, emb_bstride, M, B, D, w.partials, w.P);
  for (int s = 0; s < R; ++s) {
    hipLaunchKernelGGL(revive_pick_kernel, dim3(nb), dim3(kKmThreads), 0, st, w.Z, w.mind,
                       w.partials, w.P, B, D, s, (u64)seed, v);
    if (s + 1 < R)
      hipLaunchKernelGGL(revive_fold_kernel, dim3(w.P, nb), dim3(kKmThreads), 0, st, w.Z, w.mind,
                         rows, R, s, B, D, w.partials, w.P);
  }
  return check_launch("vq_revive");
}
