// A retrieval index compacted by Lloyd's iteration: the centroids of a singer's content frames instead of a strided
// sample of them. The arithmetic is include/svc_hip.h's (svc_index_assign, svc_index_update, svc_index_kmeans; DESIGN.md
// "Index compaction"):
//   assign: label[r] = the j smallest under (s_j, j), s_j = norms[j] - 2 dot(x_r, c_j): retrieval's own score, so the
//           distance GEMM is knn_topk (retrieve.hip) with the rows as queries and the centroids as the index, walked in
//           chunks of rows; index_label takes rank 0 of the splits' candidates, counts, and leaves the row's f32 term
//           max(|x_r|^2 + s, 0); inertia_part / inertia_final add the terms in f64 in an order fixed by N.
//   update: the exact mean. I(v) = v 2^24 is an integer for every finite f16 value, so a cluster's column sums are
//           exact in int64 and independent of the order in which its rows are met. index_hist / index_scan /
//           index_scatter group the row numbers by label (a counting sort with an integer cursor per cluster);
//           index_sum gives every cluster one workgroup per 1024 member rows, which streams whole rows in 16-byte pieces
//           (lane l takes pieces l, l + 64, ...: retrieve_blend's map) into int64 registers, adds its four waves in LDS
//           and either finishes the centroid (the f16 row, 16-byte stores) or, for a cluster of more than 1024 rows,
//           leaves its int64 partial row for index_combine. index_rownorms: the new rows' norms in svc_index_norms'
//           arithmetic, 64 rows per wave.
// Nothing here reads a value back on the host: cluster sizes decide the work inside the launches, never their grids.
#include "../../include/svc_hip.h"
#include "common.h"
#include "kernels.h"
#include "prims.h"

#pragma clang fp contract(off)

namespace svc {

namespace {

constexpr int kThreads = 256;
constexpr int kTop = 8;                 // knn_topk's candidates per row and split (retrieve.hip)
constexpr int kNoIdx = 0x7fffffff;      // its empty candidate slot
constexpr int kAllRows = 0x7fffffff;    // knn_topk's T and frames[0]: one utterance that holds every row
constexpr int kChunk = 1 << 18;         // rows per knn_topk launch (bounds the candidate scratch)
constexpr int64_t kCandRows = 1 << 20;  // rows x splits of one launch at the most (64 B each)
constexpr int kSeg = 1024;              // member rows per workgroup of index_sum
constexpr int kRed = 4096;              // inertia terms per workgroup of inertia_part
constexpr int kScan = 1024;             // threads of index_scan's one workgroup
constexpr int kMaxD = 2048;

__device__ __forceinline__ bool pair_lt(float s, int j, float s2, int j2) { return s < s2 || (s == s2 && j < j2); }

// v 2^24 of a binary16 bit pattern: m for a subnormal, (1024 + m) 2^(e - 1) otherwise, |I| < 2^40. Inf / NaN patterns
// give some integer (the caller's error)
__device__ __forceinline__ int64_t half_int(unsigned h) {
  const unsigned e = (h >> 10) & 31u, m = h & 1023u;
  const int64_t mag = e ? (int64_t)((uint64_t)(1024u | m) << (e - 1)) : (int64_t)m;
  return (h & 0x8000u) ? -mag : mag;
}

// ------------------------------------------------------------------------------------------------------------ assign
// zeroes counts (where given) and writes knn_topk's table: frames[0] = every row, sel[0] = 1
__global__ __launch_bounds__(kThreads) void index_prep_kernel(int* __restrict__ counts, int K, int* __restrict__ table) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (counts && i < K) counts[i] = 0;
  if (i == 0) table[0] = kAllRows, table[1] = 1;
}

// One wave per row of the chunk: the smallest (s, j) of the splits' rank-0 candidates is the label. |x|^2 as
// retrieve_blend sums |q|^2 (each lane its pieces' squares in column order, then the butterfly), only where terms is
// given. A row without a candidate (non-finite scores: the caller's error) is labelled 0.
__global__ __launch_bounds__(kThreads) void index_label_kernel(const f16* __restrict__ x, int M, int D, int ld, int K,
                                                               int n_splits, const float* __restrict__ cand_s,
                                                               const int* __restrict__ cand_j, int* __restrict__ labels,
                                                               int* __restrict__ counts, float* __restrict__ terms) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (r >= M) return;  // wave-uniform
  float bs = __builtin_inff();
  int bj = kNoIdx;
  for (int c = lane; c < n_splits; c += 64) {
    const int64_t o = ((int64_t)r * n_splits + c) * kTop;
    const float s = cand_s[o];
    const int j = cand_j[o];
    if (pair_lt(s, j, bs, bj)) bs = s, bj = j;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o);
    const int oj = __shfl_xor(bj, o);
    if (pair_lt(os, oj, bs, bj)) bs = os, bj = oj;
  }
  const bool ok = (unsigned)bj < (unsigned)K;
  const int label = ok ? bj : 0;
  float x2 = 0.0f;
  if (terms) {
    const uint4* row = reinterpret_cast<const uint4*>(x + (int64_t)r * ld);
    const int nchunks = D / 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (lane + 64 * c < nchunks) v = row[lane + 64 * c];
      const half8 h = __builtin_bit_cast(half8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) x2 = x2 + (float)h[e] * (float)h[e];
    }
    x2 = wave_sum(x2);
  }
  if (lane == 0) {
    labels[r] = label;
    if (counts) atomicAdd(&counts[label], 1);
    if (terms) {
      const float d = x2 + bs;
      terms[r] = d > 0.0f ? d : 0.0f;
    }
  }
}

// fixed-order tree over the workgroup's 256 partial sums
__device__ __forceinline__ double block_sum256(double a, double* sh) {
  const int t = threadIdx.x;
  sh[t] = a;
  __syncthreads();
#pragma unroll
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] = sh[t] + sh[t + o];
    __syncthreads();
  }
  return sh[0];
}

// part[b] = the f64 sum of terms [4096 b, 4096 (b + 1)): thread t adds t, t + 256, ... ascending, then the tree
__global__ __launch_bounds__(kThreads) void inertia_part_kernel(const float* __restrict__ terms, int64_t N,
                                                                double* __restrict__ part) {
  __shared__ double sh[kThreads];
  const int64_t base = (int64_t)blockIdx.x * kRed;
  double a = 0.0;
#pragma unroll
  for (int i = 0; i < kRed / kThreads; ++i) {
    const int64_t r = base + threadIdx.x + kThreads * i;
    if (r < N) a = a + (double)terms[r];
  }
  const double tot = block_sum256(a, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kThreads) void inertia_final_kernel(const double* __restrict__ part, int n,
                                                                 double* __restrict__ out) {
  __shared__ double sh[kThreads];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) a = a + part[i];
  const double tot = block_sum256(a, sh);
  if (threadIdx.x == 0) out[0] = tot;
}

// ------------------------------------------------------------------------------------------------------------ update
__global__ __launch_bounds__(kThreads) void index_hist_kernel(const int* __restrict__ labels, int64_t N, int K,
                                                              int* __restrict__ counts) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= N) return;
  const int l = labels[r];
  if ((unsigned)l < (unsigned)K) atomicAdd(&counts[l], 1);
}

// One workgroup. Cluster j has ns_j = max(1, ceil(count_j / 1024)) segments. Exclusive scans over j of count_j (offs,
// and the scatter's cursor), of ns_j - 1 (xstart: its first extra segment) and of [ns_j > 1] (its rank among the split
// clusters). pslot[j] = xstart[j] + rank: the first partial row of a split cluster. mlist[rank] = j and
// xseg[xstart[j] + i - 1] = j (segment i >= 1) let index_sum and index_combine find their cluster without a search.
// meta[0] = split clusters, meta[1] = extra segments; both are at most N / 1024.
__global__ __launch_bounds__(kScan) void index_scan_kernel(const int* __restrict__ counts, int K, int cap,
                                                           int* __restrict__ offs, int* __restrict__ cursor,
                                                           int* __restrict__ xstart, int* __restrict__ pslot,
                                                           int* __restrict__ mlist, int* __restrict__ xseg,
                                                           int* __restrict__ meta) {
  __shared__ int sc[3][kScan];
  const int t = threadIdx.x;
  const int per = (K + kScan - 1) / kScan;
  const int lo = min(K, t * per), hi = min(K, lo + per);
  int c = 0, xs = 0, m = 0;
  for (int j = lo; j < hi; ++j) {
    const int cnt = counts[j], ns = max(1, (cnt + kSeg - 1) / kSeg);
    c += cnt, xs += ns - 1, m += ns > 1;
  }
  sc[0][t] = c, sc[1][t] = xs, sc[2][t] = m;
  __syncthreads();
  for (int o = 1; o < kScan; o <<= 1) {  // inclusive Hillis-Steele
    int v0 = 0, v1 = 0, v2 = 0;
    if (t >= o) v0 = sc[0][t - o], v1 = sc[1][t - o], v2 = sc[2][t - o];
    __syncthreads();
    sc[0][t] += v0, sc[1][t] += v1, sc[2][t] += v2;
    __syncthreads();
  }
  int c0 = sc[0][t] - c, x0 = sc[1][t] - xs, m0 = sc[2][t] - m;
  for (int j = lo; j < hi; ++j) {
    const int cnt = counts[j], ns = max(1, (cnt + kSeg - 1) / kSeg);
    offs[j] = c0, cursor[j] = c0, xstart[j] = x0, pslot[j] = x0 + m0;
    if (ns > 1) {
      if (m0 < cap) mlist[m0] = j;
      for (int i = 1; i < ns; ++i)
        if (x0 + i - 1 < cap) xseg[x0 + i - 1] = j;
    }
    c0 += cnt, x0 += ns - 1, m0 += ns > 1;
  }
  if (t == kScan - 1) meta[0] = min(sc[2][t], cap), meta[1] = min(sc[1][t], cap);
}

// order[offs[l] ..]: the rows labelled l, in arrival order (the sums do not depend on it)
__global__ __launch_bounds__(kThreads) void index_scatter_kernel(const int* __restrict__ labels, int64_t N, int K,
                                                                 int* __restrict__ cursor, int* __restrict__ order) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= N) return;
  const int l = labels[r];
  if ((unsigned)l >= (unsigned)K) return;
  const int pos = atomicAdd(&cursor[l], 1);
  if ((unsigned)pos < (unsigned)N) order[pos] = (int)r;
}

// The workgroup's tail: sum[0 .. D) (LDS, the cluster's exact column sums) -> centroid j. new[c] =
// (half)(float)(((double)S / (double)count) 2^-24); count = 0 keeps prev's row. The row goes out in 16-byte pieces from
// LDS (its norm is index_rownorms' work: one thread adding D squares here held the whole workgroup for 11 us).
__device__ __forceinline__ void finish_centroid(const int64_t* sum, f16* row16, int j, int cnt, int D,
                                                const f16* prev, int ld_prev, f16* out, int ld_out) {
  const int t = threadIdx.x, nchunks = D / 8;
  if (cnt == 0) {
    for (int p = t; p < nchunks; p += kThreads)
      reinterpret_cast<uint4*>(row16)[p] = reinterpret_cast<const uint4*>(prev + (int64_t)j * ld_prev)[p];
  } else {
    const double n = (double)cnt;
    for (int el = t; el < D; el += kThreads) row16[el] = (f16)(float)(((double)sum[el] / n) * 0x1p-24);
  }
  __syncthreads();
  for (int p = t; p < nchunks; p += kThreads)
    reinterpret_cast<uint4*>(out + (int64_t)j * ld_out)[p] = reinterpret_cast<const uint4*>(row16)[p];
}

// Workgroup b < K: segment 0 of cluster b. Workgroup K + e: extra segment e (of a cluster of more than 1024 rows),
// where there is one. Wave w takes the segment's members w, w + 4, ..., two rows in flight.
__global__ __launch_bounds__(kThreads) void index_sum_kernel(
    const f16* __restrict__ x, int64_t N, int D, int ld, int K, const int* __restrict__ counts,
    const int* __restrict__ offs, const int* __restrict__ xstart, const int* __restrict__ pslot,
    const int* __restrict__ xseg, const int* __restrict__ meta, const int* __restrict__ order,
    int64_t* __restrict__ partial, int pcap, const f16* prev, int ld_prev, f16* out, int ld_out) {
  __shared__ __attribute__((aligned(16))) int64_t sum[kMaxD];
  __shared__ __attribute__((aligned(16))) f16 row16[kMaxD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int j = blockIdx.x, seg = 0;
  if (j >= K) {
    const int e = j - K;
    if (e >= meta[1]) return;  // workgroup-uniform
    j = xseg[e];
    if ((unsigned)j >= (unsigned)K) return;
    seg = e - xstart[j] + 1;
  }
  const int cnt = counts[j], off = offs[j];
  const int ns = max(1, (cnt + kSeg - 1) / kSeg);
  const int lo = seg * kSeg, hi = min(cnt, lo + kSeg);
  for (int el = t; el < D; el += kThreads) sum[el] = 0;
  __syncthreads();
  const int nchunks = D / 8;
  int64_t acc[4][8];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[c][e] = 0;
  auto fetch = [&](int m, uint4(&v)[4]) {
    int64_t row = -1;
    if (m < hi && (unsigned)(off + m) < (unsigned)N) row = order[off + m];
    const bool ok = row >= 0 && row < N;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = make_uint4(0, 0, 0, 0);  // +0: adds nothing
      if (ok && lane + 64 * c < nchunks) v[c] = reinterpret_cast<const uint4*>(x + row * ld)[lane + 64 * c];
    }
  };
  auto add = [&](const uint4(&v)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned w[4] = {v[c].x, v[c].y, v[c].z, v[c].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[c][2 * e] += half_int(w[e] & 0xffffu);
        acc[c][2 * e + 1] += half_int(w[e] >> 16);
      }
    }
  };
  for (int m = lo + wave; m < hi; m += 8) {
    uint4 va[4], vb[4];
    fetch(m, va);
    fetch(m + 4, vb);
    add(va);
    add(vb);
  }
  if (lo + wave < hi) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (lane + 64 * c < nchunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          atomicAdd(reinterpret_cast<unsigned long long*>(&sum[(lane + 64 * c) * 8 + e]),
                    (unsigned long long)acc[c][e]);
      }
  }
  __syncthreads();
  if (ns == 1) {
    finish_centroid(sum, row16, j, cnt, D, prev, ld_prev, out, ld_out);
  } else {
    const int slot = pslot[j] + seg;
    if ((unsigned)slot < (unsigned)pcap)
      for (int el = t; el < D; el += kThreads) partial[(int64_t)slot * D + el] = sum[el];
  }
}

// Workgroup m < meta[0]: the m-th cluster of more than 1024 rows: its segments' partial rows added in int64
__global__ __launch_bounds__(kThreads) void index_combine_kernel(
    int D, int K, const int* __restrict__ counts, const int* __restrict__ pslot, const int* __restrict__ mlist,
    const int* __restrict__ meta, const int64_t* __restrict__ partial, int pcap, const f16* prev,
    int ld_prev, f16* out, int ld_out) {
  __shared__ __attribute__((aligned(16))) int64_t sum[kMaxD];
  __shared__ __attribute__((aligned(16))) f16 row16[kMaxD];
  if ((int)blockIdx.x >= meta[0]) return;
  const int j = mlist[blockIdx.x];
  if ((unsigned)j >= (unsigned)K) return;
  const int cnt = counts[j], ns = (cnt + kSeg - 1) / kSeg, p0 = pslot[j];
  for (int el = threadIdx.x; el < D; el += kThreads) {
    int64_t s = 0;
    for (int i = 0; i < ns; ++i)
      if ((unsigned)(p0 + i) < (unsigned)pcap) s += partial[(int64_t)(p0 + i) * D + el];
    sum[el] = s;
  }
  __syncthreads();
  finish_centroid(sum, row16, j, cnt, D, prev, ld_prev, out, ld_out);
}

// norms[j] in svc_index_norms' arithmetic (the f64 sum of the row's squares in column order) for 64 rows per wave, with
// coalesced loads: a stage is 64 columns of the 64 rows, eight consecutive lanes reading one row's 128 bytes; every
// lane squares what it loaded in f64 (exact) into LDS, then lane l adds row l's 64 squares in column order while the
// next stage's loads are in flight. index_norms_kernel's one-row-per-thread loads touch 64 cache lines per instruction.
__global__ __launch_bounds__(64) void index_rownorms_kernel(const f16* __restrict__ x, int K, int D, int ld,
                                                            float* __restrict__ norms) {
  __shared__ __attribute__((aligned(16))) double sq[64][66];  // 528-byte rows: 16-byte aligned, four banks apart
  const int lane = threadIdx.x, r0 = blockIdx.x * 64;
  uint4 v[8];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane + 64 * i, row = c >> 3, col = c0 + (c & 7) * 8;
      v[i] = make_uint4(0, 0, 0, 0);
      if (r0 + row < K && col < D) v[i] = *reinterpret_cast<const uint4*>(x + (int64_t)(r0 + row) * ld + col);
    }
  };
  double acc = 0.0;
  fetch(0);
  for (int c0 = 0; c0 < D; c0 += 64) {
    __syncthreads();  // the previous stage's reads
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane + 64 * i;
      const half8 h = __builtin_bit_cast(half8, v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double d = (double)(float)h[e];
        sq[c >> 3][(c & 7) * 8 + e] = d * d;
      }
    }
    __syncthreads();
    if (c0 + 64 < D) fetch(c0 + 64);
    const int n = min(64, D - c0);
    for (int e = 0; e < n; e += 2) {  // D is a multiple of 8
      const double2 p = *reinterpret_cast<const double2*>(&sq[lane][e]);
      acc += p.x;
      acc += p.y;
    }
  }
  if (r0 + lane < K) norms[r0 + lane] = (float)acc;
}

// ------------------------------------------------------------------------------------------------------------ k-means
// centroid i = row floor(i N / K): one wave per centroid
__global__ __launch_bounds__(kThreads) void index_init_kernel(const f16* __restrict__ x, int64_t N, int D, int ld, int K,
                                                              f16* __restrict__ cent, int ld_cent) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (i >= K) return;
  const int64_t src = (int64_t)i * N / K;
  for (int p = lane; p < D / 8; p += 64)
    reinterpret_cast<uint4*>(cent + (int64_t)i * ld_cent)[p] = reinterpret_cast<const uint4*>(x + src * ld)[p];
}

// ------------------------------------------------------------------------------------------------------------ host
// rows per knn_topk launch, and its splits at that many rows
int chunk_rows(int64_t N, int K, int* splits) {
  int M = (int)std::min<int64_t>(N, kChunk);
  int sp = retrieve_splits(M, K);
  if ((int64_t)M * sp > kCandRows) {
    M = std::max(128, (int)(kCandRows / sp) & ~127);
    sp = retrieve_splits(M, K);
  }
  *splits = sp;
  return M;
}

struct AssignWs {
  float* cand_s = nullptr;
  int* cand_j = nullptr;
  int* table = nullptr;
  float* terms = nullptr;
  double* part = nullptr;
};

void lay_assign(Arena& a, int64_t N, int K, bool inertia, AssignWs& w) {
  int sp = 1;
  const int M = chunk_rows(N, K, &sp);
  // a shorter last chunk may be split more ways, never into more candidates than 128 x 64 per query tile allows
  size_t rows = (size_t)M * sp;
  const int64_t last = N % M;
  if (last) rows = std::max(rows, (size_t)last * retrieve_splits((int)last, K));
  w.cand_s = a.get<float>(rows * kTop);
  w.cand_j = a.get<int>(rows * kTop);
  w.table = a.get<int>(2);
  w.terms = inertia ? a.get<float>((size_t)N) : nullptr;
  w.part = inertia ? a.get<double>((size_t)cdiv64(N, kRed)) : nullptr;
}

int run_assign(const f16* x, int64_t N, int D, int ld, const f16* cent, const float* cnorms, int K, int ld_cent,
               int* labels, int* counts, double* inertia, const AssignWs& w, hipStream_t s) {
  {
    const int tok = prof_begin("index_prep", 0.0, (counts ? K : 0) * 4.0 + 8.0, s);
    hipLaunchKernelGGL(index_prep_kernel, dim3((unsigned)cdiv(counts ? K : 1, kThreads)), dim3(kThreads), 0, s, counts, K,
                       w.table);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  int sp0 = 1;
  const int chunk = chunk_rows(N, K, &sp0);
  for (int64_t r0 = 0; r0 < N; r0 += chunk) {
    const int M = (int)std::min<int64_t>(chunk, N - r0);
    const int sp = M == chunk ? sp0 : retrieve_splits(M, K);
    const f16* xr = x + r0 * ld;
    if (int st = knn_topk(xr, M, kAllRows, D, ld, w.table, 1, cent, cnorms, K, ld_cent, sp, w.cand_s, w.cand_j, s))
      return st;
    const int tok = prof_begin("index_label", inertia ? 2.0 * M * D : 0.0,
                               (double)M * sp * 8.0 + (inertia ? (double)M * D * 2.0 : 0.0), s);
    hipLaunchKernelGGL(index_label_kernel, dim3((unsigned)cdiv(M, kThreads / 64)), dim3(kThreads), 0, s, xr, M, D, ld, K,
                       sp, w.cand_s, w.cand_j, labels + r0, counts, inertia ? w.terms + r0 : nullptr);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  if (inertia) {
    const int nb = (int)cdiv64(N, kRed);
    const int tok = prof_begin("inertia_sum", (double)N, (double)N * 4.0, s);
    hipLaunchKernelGGL(inertia_part_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, w.terms, N, w.part);
    hipLaunchKernelGGL(inertia_final_kernel, dim3(1), dim3(kThreads), 0, s, w.part, nb, inertia);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  return SVC_OK;
}

struct UpdateWs {
  int *counts = nullptr, *offs = nullptr, *cursor = nullptr, *xstart = nullptr, *pslot = nullptr, *mlist = nullptr,
      *xseg = nullptr, *meta = nullptr, *order = nullptr;
  int64_t* partial = nullptr;
  int cap = 0, pcap = 0;
};

void lay_update(Arena& a, int64_t N, int D, int K, bool own_counts, UpdateWs& w) {
  w.cap = (int)(N / kSeg) + 1;       // split clusters, and extra segments, at the most (+ 1: never an empty buffer)
  w.pcap = 2 * (int)(N / kSeg) + 2;  // their partial rows: every segment of every split cluster
  w.counts = own_counts ? a.get<int>((size_t)K) : nullptr;
  w.offs = a.get<int>((size_t)K);
  w.cursor = a.get<int>((size_t)K);
  w.xstart = a.get<int>((size_t)K);
  w.pslot = a.get<int>((size_t)K);
  w.mlist = a.get<int>((size_t)w.cap);
  w.xseg = a.get<int>((size_t)w.cap);
  w.meta = a.get<int>(2);
  w.order = a.get<int>((size_t)N);
  w.partial = N > kSeg ? a.get<int64_t>((size_t)w.pcap * D) : nullptr;
  if (N <= kSeg) w.pcap = 0;  // no cluster can be split
}

int run_update(const f16* x, int64_t N, int D, int ld, const int* labels, int K, const f16* prev, int ld_prev, f16* out,
               int ld_out, float* norms_out, int* counts, const UpdateWs& w, hipStream_t s) {
  if (!counts) counts = w.counts;
  const unsigned rb = (unsigned)cdiv64(N, kThreads);
  int tok = prof_begin("index_hist", 0.0, (double)N * 4.0 + K * 4.0, s);
  SVC_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)K * sizeof(int), s));
  hipLaunchKernelGGL(index_hist_kernel, dim3(rb), dim3(kThreads), 0, s, labels, N, K, counts);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  tok = prof_begin("index_scan", 0.0, K * 20.0, s);
  hipLaunchKernelGGL(index_scan_kernel, dim3(1), dim3(kScan), 0, s, counts, K, w.cap, w.offs, w.cursor, w.xstart, w.pslot,
                     w.mlist, w.xseg, w.meta);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  tok = prof_begin("index_scatter", 0.0, (double)N * 8.0, s);
  hipLaunchKernelGGL(index_scatter_kernel, dim3(rb), dim3(kThreads), 0, s, labels, N, K, w.cursor, w.order);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  const int extra = (int)(N / kSeg);
  tok = prof_begin("index_sum", (double)N * D, ((double)N + K) * D * 2.0, s);
  hipLaunchKernelGGL(index_sum_kernel, dim3((unsigned)(K + extra)), dim3(kThreads), 0, s, x, N, D, ld, K, counts, w.offs,
                     w.xstart, w.pslot, w.xseg, w.meta, w.order, w.partial, w.pcap, prev, ld_prev, out, ld_out);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  if (extra > 0) {
    tok = prof_begin("index_combine", 0.0, (double)w.pcap * D * 8.0, s);
    hipLaunchKernelGGL(index_combine_kernel, dim3((unsigned)extra), dim3(kThreads), 0, s, D, K, counts, w.pslot, w.mlist,
                       w.meta, w.partial, w.pcap, prev, ld_prev, out, ld_out);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  tok = prof_begin("index_rownorms", 2.0 * K * D, (double)K * D * 2.0, s);
  hipLaunchKernelGGL(index_rownorms_kernel, dim3((unsigned)cdiv(K, 64)), dim3(64), 0, s, out, K, D, ld_out, norms_out);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

}  // namespace

int index_assign(const f16* x, int64_t N, int D, int ld, const f16* cent, const float* cnorms, int K, int ld_cent,
                 int* labels, int* counts, double* inertia, Arena& ws, hipStream_t s) {
  AssignWs w;
  if (int st = ws.plan([&](Arena& a) { lay_assign(a, N, K, inertia != nullptr, w); })) return st;
  return run_assign(x, N, D, ld, cent, cnorms, K, ld_cent, labels, counts, inertia, w, s);
}

int index_update(const f16* x, int64_t N, int D, int ld, const int* labels, int K, const f16* prev, int ld_prev, f16* out,
                 int ld_out, float* norms_out, int* counts, Arena& ws, hipStream_t s) {
  UpdateWs w;
  if (int st = ws.plan([&](Arena& a) { lay_update(a, N, D, K, counts == nullptr, w); })) return st;
  return run_update(x, N, D, ld, labels, K, prev, ld_prev, out, ld_out, norms_out, counts, w, s);
}

int index_kmeans(const f16* x, int64_t N, int D, int ld, int K, int iters, f16* cent, int ld_cent, float* cnorms,
                 int* labels, int* counts, double* inertia, Arena& ws, hipStream_t s) {
  AssignWs aw;
  UpdateWs uw;
  int* own_labels = nullptr;
  if (int st = ws.plan([&](Arena& a) {
        lay_assign(a, N, K, inertia != nullptr, aw);
        lay_update(a, N, D, K, true, uw);
        own_labels = labels ? nullptr : a.get<int>((size_t)N);
      }))
    return st;
  if (!labels) labels = own_labels;
  {
    const int tok = prof_begin("index_init", 0.0, (double)K * D * 4.0, s);
    hipLaunchKernelGGL(index_init_kernel, dim3((unsigned)cdiv(K, kThreads / 64)), dim3(kThreads), 0, s, x, N, D, ld, K,
                       cent, ld_cent);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  if (int st = index_norms(cent, K, D, ld_cent, cnorms, s)) return st;
  for (int it = 0; it < iters; ++it) {
    if (int st = run_assign(x, N, D, ld, cent, cnorms, K, ld_cent, labels, nullptr, inertia ? inertia + it : nullptr, aw,
                            s))
      return st;
    if (int st = run_update(x, N, D, ld, labels, K, cent, ld_cent, cent, ld_cent, cnorms, nullptr, uw, s)) return st;
  }
  return run_assign(x, N, D, ld, cent, cnorms, K, ld_cent, labels, counts, inertia ? inertia + iters : nullptr, aw, s);
}

}  // namespace svc
