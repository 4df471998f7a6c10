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

// Fold centroid s (row seed_rows[b][s]) into mind; partials[b][part] = the
// part's sum of q.
__global__ void __launch_bounds__(kKmThreads)
kmeans_mind_kernel(const float* __restrict__ Z, float* __restrict__ mind,
                   const float* __restrict__ cent, int ldw, int64_t cen_bstride,
                   const int* __restrict__ seed_rows, int M, int s, int B, int W,
                   u64* __restrict__ partials, int P) {
  __shared__ u64 wsum[kKmWaves];
  const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float c[kKmMaxW];
  const float* cp = cent + (int64_t)b * cen_bstride + (int64_t)s * ldw;
#pragma unroll
  for (int k = 0; k < kKmMaxW; ++k) c[k] = k < W ? cp[k] : 0.f;
  const float cc = km_sumsq(c, W);
  const int istar = seed_rows[(int64_t)b * M + s];
  const float* zb = Z + (int64_t)b * B * W;
  float* mb = mind + (int64_t)b * B;
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
  if (tid == 0) partials[(int64_t)b * P + part] = total;
}

// Step s of branch b = blockIdx.x: the D^2 draw over the part sums and the
// chosen part's rows; writes seed_rows[b][s] and centroid[b][s].
__global__ void __launch_bounds__(kKmThreads)
kmeans_pick_kernel(const float* __restrict__ Z, const float* __restrict__ mind,
                   const u64* __restrict__ partials, int P, int B, int W, int M, int s, u64 seed,
                   float* __restrict__ cent, int ldw, int64_t cen_bstride,
                   int* __restrict__ seed_rows) {
  __shared__ u64 wsum[kKmWaves];
  __shared__ u64 sh_t;
  __shared__ int sh_part, sh_row;
  const int b = blockIdx.x, tid = threadIdx.x;
  const u64 r = km_draw(seed, b, s);
  const u64* pb = partials + (int64_t)b * P;
  const float* mb = mind + (int64_t)b * B;
  if (tid == 0) sh_part = -1, sh_row = -1;
  u64 T = 0;
  if (s > 0) {
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
