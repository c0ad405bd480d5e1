// Feature retrieval (RVC's feature index, `index_rate`): every content frame of the source is blended with a
// distance-weighted mean of its k nearest content frames from the target singer's own recordings. The arithmetic is
// include/svc_hip.h's (svc_index_norms, svc_content_retrieve; DESIGN.md "Feature retrieval"):
//   s_j  = norms[j] - 2 dot(q, x_j)            f16 products accumulated in f32 on v_mfma_f32_16x16x32_f16, K ascending
//   pick = the min(k, N) smallest under the total order (s_j, j)
//   d2_i = max(|q|^2 + s_i, floor), w_i = (1 / d2_i) / sum_i (1 / d2_i), y = sum_i w_i x_i (f32 fma, rank order)
//   out  = round16(rate y + (1 - rate) q)
// Three kernels. index_norms: one thread per index row. knn_topk: the distance GEMM with the selection as its epilogue;
// the M x N scores live in accumulators only. retrieve_blend: merges the index splits' candidates, weights, gathers and
// blends, one wave per row. The selection is by a total order, so its result does not depend on the tiling or on the
// number of index splits; the blend's f32 sums run in an order fixed by D and the ranks alone.
#include "../../include/svc_hip.h"
#include "common.h"
#include "kernels.h"
#include "prims.h"

#pragma clang fp contract(off)

namespace svc {

namespace {

constexpr int kThreads = 256;
constexpr int kQT = 128;   // queries per workgroup: 32 per wave, two 16-column MFMA blocks
constexpr int kNT = 128;   // index rows per tile: eight 16-row MFMA blocks, every wave takes all of them
constexpr int kKT = 64;    // halves of K per LDS stage: 128-byte rows (prims.h sw128), two MFMA k-steps
constexpr int kTop = 8;    // candidates kept per query (the largest k)
constexpr int kNoIdx = 0x7fffffff;  // an empty candidate slot: (+inf, kNoIdx), after every real (s, j)
constexpr int kMaxSplits = 64;

__device__ __forceinline__ bool pair_lt(float s, int j, float s2, int j2) { return s < s2 || (s == s2 && j < j2); }

// norms[j] = (float) sum_c (double)x[j][c]^2, columns ascending: every square is exact in f64
__global__ __launch_bounds__(kThreads) void index_norms_kernel(const f16* __restrict__ x, int64_t N, int D, int ld,
                                                               float* __restrict__ norms) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= N) return;
  const uint4* row = reinterpret_cast<const uint4*>(x + j * ld);
  double acc = 0.0;
  for (int c = 0; c < D / 8; ++c) {
    const half8 h = __builtin_bit_cast(half8, row[c]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double v = (double)(float)h[e];
      acc += v * v;
    }
  }
  norms[j] = (float)acc;
}

// does row r = b T + t of the batch take part?
__device__ __forceinline__ bool row_live(int r, int T, const int* __restrict__ frames, const int* __restrict__ sel) {
  const int b = r / T, t = r - b * T;
  return sel[b] != 0 && t < frames[b];
}

// Workgroup (query tile, index split): the transposed product S^T = X Q^T over the split's index tiles. Index rows are
// the MFMA rows and queries the MFMA columns, so by the C/D map (col = lane & 15, row = 4 (lane >> 4) + reg) a lane
// owns one query of each of its wave's two 16-column blocks and sees four index rows of it per MFMA. Its running top-8
// of that query is a sorted register list; a lane meets its candidates in ascending j, so "s below the list's worst"
// is the (s, j) order. The four lane groups of a query are merged once at the end through LDS.
// cand_s / cand_j [M][n_splits][8]: the split's eight smallest (s, j) of each row, ascending, empty slots last.
__global__ __launch_bounds__(kThreads) void knn_topk_kernel(const f16* __restrict__ q, int M, int T, int D, int ld,
                                                            const int* __restrict__ frames,
                                                            const int* __restrict__ sel, const f16* __restrict__ x,
                                                            const float* __restrict__ norms, int N, int ld_index,
                                                            int n_splits, float* __restrict__ cand_s,
                                                            int* __restrict__ cand_j) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kNT + kQT) * 128];
  __shared__ __attribute__((aligned(16))) float nrm[kNT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int qtile = blockIdx.x / n_splits, split = blockIdx.x - qtile * n_splits;
  const int r0 = qtile * kQT;
  {  // a tile none of whose rows takes part (padding, unselected clips) is not computed: nothing reads its candidates
    int live = 0;
    if (tid < kQT && r0 + tid < M) live = row_live(r0 + tid, T, frames, sel) ? 1 : 0;
    if (!__syncthreads_or(live)) return;
  }
  const int tiles = (N + kNT - 1) / kNT;
  const int t_lo = (int)((int64_t)split * tiles / n_splits), t_hi = (int)((int64_t)(split + 1) * tiles / n_splits);
  unsigned char* const ldsA = lds;
  unsigned char* const ldsB = lds + kNT * 128;

  float ls[2][kTop];
  int lj[2][kTop];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int i = 0; i < kTop; ++i) ls[qb][i] = __builtin_inff(), lj[qb][i] = kNoIdx;

  const int nk = (D + kKT - 1) / kKT;
  // this thread's four 16-byte chunks of each image: chunk id c = tid + 256 i is row c >> 3, k-chunk c & 7
  uint4 ra[4], rb[4];
  for (int tile = t_lo; tile < t_hi; ++tile) {
    const int j0 = tile * kNT;
    auto fetch = [&](int ks) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = tid + kThreads * i, row = c >> 3, kcol = ks * kKT + (c & 7) * 8;
        ra[i] = make_uint4(0, 0, 0, 0);
        rb[i] = make_uint4(0, 0, 0, 0);
        if (kcol < D) {  // D is a multiple of 8: a chunk lies wholly inside or outside the row
          if (row < N - j0) ra[i] = *reinterpret_cast<const uint4*>(x + (int64_t)(j0 + row) * ld_index + kcol);
          if (row < M - r0) rb[i] = *reinterpret_cast<const uint4*>(q + (int64_t)(r0 + row) * ld + kcol);
        }
      }
    };
    floatx4 acc[8][2];
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) acc[ib][qb] = floatx4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int ks = 0; ks < nk; ++ks) {
      __syncthreads();  // the previous stage's fragment reads, and the previous tile's reads of nrm
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = tid + kThreads * i, row = c >> 3, off = row * 128 + sw128(row, c & 7) * 16;
        *reinterpret_cast<uint4*>(ldsA + off) = ra[i];
        *reinterpret_cast<uint4*>(ldsB + off) = rb[i];
      }
      if (ks == 0 && tid < kNT) nrm[tid] = tid < N - j0 ? norms[j0 + tid] : __builtin_inff();
      __syncthreads();
      if (ks + 1 < nk) fetch(ks + 1);  // in flight under the MFMAs
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int kv = kk * 4 + g;
        half8 bq[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          const int row = wave * 32 + qb * 16 + l15;
          bq[qb] = *reinterpret_cast<const half8*>(ldsB + row * 128 + sw128(row, kv) * 16);
        }
#pragma unroll
        for (int ib = 0; ib < 8; ++ib) {
          const int row = ib * 16 + l15;
          const half8 ax = *reinterpret_cast<const half8*>(ldsA + row * 128 + sw128(row, kv) * 16);
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) acc[ib][qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ax, bq[qb], acc[ib][qb], 0, 0, 0);
        }
      }
    }
    // selection epilogue: index row j0 + 16 ib + 4 g + e, ascending in (ib, e). A row past N has norm +inf and a zero
    // product, so it is never below the list's worst
#pragma unroll
    for (int ib = 0; ib < 8; ++ib) {
      const float4 n4 = *reinterpret_cast<const float4*>(&nrm[ib * 16 + 4 * g]);
      const float nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + ib * 16 + 4 * g + e;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          const float s = nv[e] - 2.0f * acc[ib][qb][e];
          if (s < ls[qb][kTop - 1]) {
            ls[qb][kTop - 1] = s;
            lj[qb][kTop - 1] = j;
#pragma unroll
            for (int i = kTop - 1; i > 0; --i) {
              const bool sw = ls[qb][i] < ls[qb][i - 1];  // an equal s stays behind: it has the higher j
              const float a = ls[qb][i], b = ls[qb][i - 1];
              const int ja = lj[qb][i], jb = lj[qb][i - 1];
              ls[qb][i - 1] = sw ? a : b;
              ls[qb][i] = sw ? b : a;
              lj[qb][i - 1] = sw ? ja : jb;
              lj[qb][i] = sw ? jb : ja;
            }
          }
        }
      }
    }
  }
  // the four lane groups' lists of each query -> LDS [query][group][8], then one thread per query merges them
  __syncthreads();
  float* const mS = reinterpret_cast<float*>(lds);
  int* const mJ = reinterpret_cast<int*>(lds + kQT * 4 * kTop * 4);
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int base = ((wave * 32 + qb * 16 + l15) * 4 + g) * kTop;
#pragma unroll
    for (int i = 0; i < kTop; ++i) mS[base + i] = ls[qb][i], mJ[base + i] = lj[qb][i];
  }
  __syncthreads();
  if (tid < kQT && r0 + tid < M) {
    const int base = tid * 4 * kTop;
    int h0 = 0, h1 = 0, h2 = 0, h3 = 0;
    const int64_t o = ((int64_t)(r0 + tid) * n_splits + split) * kTop;
    for (int i = 0; i < kTop; ++i) {
      float bs = __builtin_inff();
      int bj = kNoIdx, bg = -1;
      auto consider = [&](int gg, int hh) {
        if (hh < kTop) {
          const float s = mS[base + gg * kTop + hh];
          const int j = mJ[base + gg * kTop + hh];
          if (pair_lt(s, j, bs, bj)) bs = s, bj = j, bg = gg;
        }
      };
      consider(0, h0);
      consider(1, h1);
      consider(2, h2);
      consider(3, h3);
      h0 += bg == 0, h1 += bg == 1, h2 += bg == 2, h3 += bg == 3;
      cand_s[o + i] = bs;
      cand_j[o + i] = bj;
    }
  }
}

// One wave per row r. A live row: the k smallest of its n_splits x 8 candidates by (s, j), one wave-wide minimum per
// rank (each the smallest pair above the previous rank's: the pairs are distinct), then the weights and the blend over
// 16-byte row pieces, lane l taking pieces l, l + 64, ... (at most four: D <= 2048). The lane that writes a piece of
// `out` is the one that read that piece of q, after the whole wave has read the row for |q|^2, so out may be q.
// |q|^2: each lane adds its pieces' squares in column order, then the 64-lane butterfly: an order fixed by D.
__global__ __launch_bounds__(kThreads) void retrieve_blend_kernel(
    const f16* q, int M, int T, int D, int ld, const int* __restrict__ frames, const int* __restrict__ sel,
    const f16* __restrict__ x, int N, int ld_index, int n_splits, const float* __restrict__ cand_s,
    const int* __restrict__ cand_j, int k, float rate, float rate1, float dist_floor, f16* out, int ld_out, int inplace,
    int* __restrict__ idx_out, float* __restrict__ dist_out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (r >= M) return;  // wave-uniform
  const int b = r / T, t = r - b * T;
  const bool selected = sel[b] != 0;
  const int nchunks = D / 8;
  const uint4* qrow = reinterpret_cast<const uint4*>(q + (int64_t)r * ld);
  uint4* orow = reinterpret_cast<uint4*>(out + (int64_t)r * ld_out);
  if (!selected || t >= frames[b]) {
    if (lane < k) {
      if (idx_out) idx_out[(int64_t)r * k + lane] = -1;
      if (dist_out) dist_out[(int64_t)r * k + lane] = 0.0f;
    }
    if (selected) {
      for (int c = lane; c < nchunks; c += 64) orow[c] = make_uint4(0, 0, 0, 0);
    } else if (!inplace) {
      for (int c = lane; c < nchunks; c += 64) orow[c] = qrow[c];
    }
    return;
  }
  uint4 qc[4];
  float q2 = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    qc[c] = make_uint4(0, 0, 0, 0);
    if (lane + 64 * c < nchunks) qc[c] = qrow[lane + 64 * c];
    const half8 h = __builtin_bit_cast(half8, qc[c]);
#pragma unroll
    for (int e = 0; e < 8; ++e) q2 = q2 + (float)h[e] * (float)h[e];
  }
  q2 = wave_sum(q2);
  // ranks
  float ss[kTop];
  int sj[kTop];
  const int ncand = n_splits * kTop;
  const int64_t cbase = (int64_t)r * ncand;
  float ps = -__builtin_inff();
  int pj = -1;
  int k_eff = 0;
#pragma unroll
  for (int i = 0; i < kTop; ++i) {
    ss[i] = 0.0f;
    sj[i] = kNoIdx;
    if (i < k) {
      float bs = __builtin_inff();
      int bj = kNoIdx;
      for (int c = lane; c < ncand; c += 64) {
        const float s = cand_s[cbase + c];
        const int j = cand_j[cbase + c];
        if (j != kNoIdx && pair_lt(ps, pj, s, j) && pair_lt(s, j, bs, bj)) bs = s, bj = j;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(bs, o);
        const int oj = __shfl_xor(bj, o);
        if (pair_lt(os, oj, bs, bj)) bs = os, bj = oj;
      }
      if ((unsigned)bj < (unsigned)N) {  // a real candidate (always a row of the index)
        ss[i] = bs, sj[i] = bj;
        ps = bs, pj = bj;
        k_eff = i + 1;
      } else {
        ps = __builtin_inff(), pj = kNoIdx;  // nothing is left: the later ranks stay empty
      }
    }
  }
  // distances and weights, ranks ascending
  float d2[kTop], w[kTop];
  float wsum = 0.0f;
#pragma unroll
  for (int i = 0; i < kTop; ++i) {
    d2[i] = 0.0f, w[i] = 0.0f;
    if (i < k_eff) {
      const float d = q2 + ss[i];
      d2[i] = d > dist_floor ? d : dist_floor;
      w[i] = 1.0f / d2[i];
      wsum = wsum + w[i];
    }
  }
#pragma unroll
  for (int i = 0; i < kTop; ++i)
    if (i < k_eff) w[i] = w[i] / wsum;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kTop; ++i)
      if (i < k) {
        if (idx_out) idx_out[(int64_t)r * k + i] = i < k_eff ? sj[i] : -1;
        if (dist_out) dist_out[(int64_t)r * k + i] = i < k_eff ? d2[i] : 0.0f;
      }
  }
  // blend
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int ch = lane + 64 * c;
    if (ch >= nchunks) break;
    const half8 qh = __builtin_bit_cast(half8, qc[c]);
    if (rate == 0.0f) {  // q's own bits (0 * y + q would turn -0 into +0)
      orow[ch] = qc[c];
      continue;
    }
    float y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kTop; ++i)
      if (i < k_eff) {
        const half8 xh = __builtin_bit_cast(
            half8, *reinterpret_cast<const uint4*>(x + (int64_t)sj[i] * ld_index + (int64_t)ch * 8));
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = fmaf(w[i], (float)xh[e], y[e]);
      }
    half8 oh;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float a = rate * y[e], bq = rate1 * (float)qh[e];
      oh[e] = (f16)(a + bq);
    }
    orow[ch] = __builtin_bit_cast(uint4, oh);
  }
}

}  // namespace

int index_norms(const f16* x, int64_t N, int D, int ld, float* norms, hipStream_t s) {
  const int tok = prof_begin("index_norms", 2.0 * (double)N * D, (double)N * D * 2.0, s);
  hipLaunchKernelGGL(index_norms_kernel, dim3((unsigned)cdiv64(N, kThreads)), dim3(kThreads), 0, s, x, N, D, ld, norms);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

// index splits of a call: tune.retrieve_splits when set, else enough workgroups for three per CU of a 256-CU part;
// never more than the index has tiles
int retrieve_splits(int M, int64_t N) {
  const int qtiles = cdiv(M, kQT), tiles = cdiv(N, kNT);
  const int forced = tuning().retrieve_splits;
  const int want = forced > 0 ? forced : cdiv(768, qtiles);
  return std::max(1, std::min(std::min(want, tiles), kMaxSplits));
}

// The distance GEMM with the selection epilogue, as one launch: cand_s / cand_j [M][n_splits][8] (content_retrieve's
// queries; index_assign's rows against the centroids, index_kmeans.hip)
int knn_topk(const f16* q, int M, int T, int D, int ld, const int* table, int B, const f16* x, const float* norms, int N,
             int ld_index, int n_splits, float* cand_s, int* cand_j, hipStream_t s) {
  const int qtiles = cdiv(M, kQT);
  const int tok = prof_begin("knn_topk", 2.0 * M * (double)N * D, ((double)M + (double)N * qtiles) * D * 2.0, s);
  hipLaunchKernelGGL(knn_topk_kernel, dim3((unsigned)(qtiles * n_splits)), dim3(kThreads), 0, s, q, M, T, D, ld, table,
                     table + B, x, norms, N, ld_index, n_splits, cand_s, cand_j);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

// table (device): int32 frames[B], then int32 sel[B], staged by the caller. The candidates come from ws.
int content_retrieve(const f16* q, int B, int T, int D, int ld, const int* table, const f16* x, const float* norms,
                     int N, int ld_index, int k, double rate, double dist_floor, f16* out, int ld_out, int* idx_out,
                     float* dist_out, Arena& ws, hipStream_t s) {
  const int M = B * T;
  const int n_splits = retrieve_splits(M, N);
  float* cand_s = nullptr;
  int* cand_j = nullptr;
  if (int st = ws.plan([&](Arena& a) {
        cand_s = a.get<float>((size_t)M * n_splits * kTop);
        cand_j = a.get<int>((size_t)M * n_splits * kTop);
      }))
    return st;
  const int* frames = table;
  const int* sel = table + B;
  if (int st = knn_topk(q, M, T, D, ld, table, B, x, norms, N, ld_index, n_splits, cand_s, cand_j, s)) return st;
  const int tok = prof_begin("retrieve_blend", 2.0 * M * (double)k * D, (double)M * (k + 2.0) * D * 2.0, s);
  hipLaunchKernelGGL(retrieve_blend_kernel, dim3((unsigned)cdiv(M, kThreads / 64)), dim3(kThreads), 0, s, q, M, T, D, ld,
                     frames, sel, x, N, ld_index, n_splits, cand_s, cand_j, k, (float)rate, (float)(1.0 - rate),
                     (float)dist_floor, out, ld_out, out == q ? 1 : 0, idx_out, dist_out);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

}  // namespace svc
