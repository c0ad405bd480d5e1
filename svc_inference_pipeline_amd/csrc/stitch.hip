// Long-form conversion's join: overlapping chunks of a song, converted as separate utterances, are aligned by SOLA and
// crossfaded into one waveform. Two launches whatever the number of chunks; the arithmetic is audio.stitch's (DESIGN.md
// "Long-form conversion"), with X = xfade, R = search and d_b the displacement of chunk b (0 for an unjoined chunk):
//   chunk b plays row sample lead[b] + d_b + j at out[out_off[b] + j], j < body[b]
//   a joined chunk's predecessor continues as a_j = rows[b-1][lead[b-1] + d_{b-1} + body[b-1] + j], j < X
//   candidate d in [-R, R) (d = 0 alone when R = 0), c_j(d) = rows[b][lead[b] + d + j]:
//     nom(d) = sum_j (double)a_j (double)c_j(d), den(d) = sum_j (double)c_j(d)^2, j ascending from 0
//     q(d)   = nom |nom| / (den + eps)
//   d_b = the candidate with the greatest q, then the smallest |d|, then the greatest d
//   out[out_off[b] + j] = (float)(a_j + w_j (c_j(d_b) - a_j)), w_j = (j + 0.5) / X, for j < X; the row sample from there
// Every product of two f32 values is exact in f64, so a fused multiply-add rounds once where the host rounds once: the
// sums are the host's bit for bit, and so are q and the displacements. The crossfade is written as the host writes it,
// one IEEE operation after the other: no contraction in this file.
#include <algorithm>
#include <vector>

#include "../../include/svc_hip.h"
#include "common.h"
#include "kernels.h"
#include "prims.h"

#pragma clang fp contract(off)

namespace svc {

namespace {

constexpr int kWriteThreads = 256;
constexpr int kSpan = 2048;         // body samples of one chunk per write block: two 16-byte chunks per thread
constexpr int kSeamThreads = 1024;  // at most; one candidate per thread up to there
constexpr int kXfadeMax = 8192, kSearchMax = 1024;
constexpr int64_t kLenMax = (int64_t)1 << 40;  // samples of a row or of the output: sums of a few never overflow

// one chunk of the staged table
struct StitchChunk {
  const float* row;  // n usable samples
  int64_t n, lead, body, out_off;
  int32_t joined, pad_;
};

// the order of the candidates: a before b
__device__ __forceinline__ bool better(double qa, int da, double qb, int db) {
  if (qa > qb) return true;
  if (!(qa == qb)) return false;
  const int ma = da < 0 ? -da : da, mb = db < 0 ? -db : db;
  return ma < mb || (ma == mb && da > db);
}

// shift[b] = d_b for every chunk of the song that starts at chunk first[blockIdx.x] (and shift_out[b], q_out[b][.]
// where given). One workgroup per song: seam b needs d_{b-1}, so a song's seams are walked in order. Per seam both
// windows are staged in LDS (the predecessor's X samples, then this chunk's X + 2R - 1), candidate k = d + R belongs to
// thread k (k + blockDim, ... beyond 1024 candidates), which sums over j ascending; then the arg-max under better()
// through the 64-lane butterfly and the waves' winners in LDS. A thread without a candidate, or whose q are all NaN,
// carries (-inf, d = 0): whatever the samples hold, the winner is one of the candidates.
__global__ __launch_bounds__(kSeamThreads) void stitch_seams_kernel(const StitchChunk* __restrict__ ch,
                                                                    const int32_t* __restrict__ first, int B, int X, int R,
                                                                    double eps, int32_t* __restrict__ shift,
                                                                    int32_t* __restrict__ shift_out,
                                                                    double* __restrict__ q_out) {
  extern __shared__ __align__(16) unsigned char stitch_sm[];
  float* a_s = reinterpret_cast<float*>(stitch_sm);  // [X rounded up to 4]
  float* c_s = a_s + ((X + 3) & ~3);                 // [X + nc - 1]
  __shared__ double wave_q[kSeamThreads / 64];
  __shared__ int wave_d[kSeamThreads / 64];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nc = R > 0 ? 2 * R : 1;
  int b = first[blockIdx.x];
  if (tid == 0) {
    shift[b] = 0;
    if (shift_out) shift_out[b] = 0;
  }
  if (q_out)
    for (int k = tid; k < nc; k += nt) q_out[(int64_t)b * nc + k] = 0.0;
  int d_prev = 0;
  for (++b; b < B && ch[b].joined; ++b) {
    const float* pa = ch[b - 1].row + (ch[b - 1].lead + d_prev + ch[b - 1].body);
    const float* pc = ch[b].row + (ch[b].lead - R);
    for (int i = tid; i < X; i += nt) a_s[i] = pa[i];
    for (int i = tid; i < X + nc - 1; i += nt) c_s[i] = pc[i];
    __syncthreads();
    double bq = -__builtin_inf();
    int bd = 0;
    for (int k = tid; k < nc; k += nt) {
      const float* cw = c_s + k;
      double nom = 0.0, den = 0.0;
      int j = 0;
      for (; j + 4 <= X; j += 4) {
        const float4 a4 = *reinterpret_cast<const float4*>(a_s + j);
        const double c0 = (double)cw[j], c1 = (double)cw[j + 1], c2 = (double)cw[j + 2], c3 = (double)cw[j + 3];
        nom = __builtin_fma((double)a4.x, c0, nom), den = __builtin_fma(c0, c0, den);
        nom = __builtin_fma((double)a4.y, c1, nom), den = __builtin_fma(c1, c1, den);
        nom = __builtin_fma((double)a4.z, c2, nom), den = __builtin_fma(c2, c2, den);
        nom = __builtin_fma((double)a4.w, c3, nom), den = __builtin_fma(c3, c3, den);
      }
      for (; j < X; ++j) {
        const double cj = (double)cw[j];
        nom = __builtin_fma((double)a_s[j], cj, nom), den = __builtin_fma(cj, cj, den);
      }
      const double q = (nom * fabs(nom)) / (den + eps);
      if (q_out) q_out[(int64_t)b * nc + k] = q;
      if (better(q, k - R, bq, bd)) bq = q, bd = k - R;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double oq = __shfl_xor(bq, o);
      const int od = __shfl_xor(bd, o);
      if (better(oq, od, bq, bd)) bq = oq, bd = od;
    }
    if ((tid & 63) == 0) wave_q[tid >> 6] = bq, wave_d[tid >> 6] = bd;
    __syncthreads();  // also: every read of the two windows lies before it
    bq = wave_q[0], bd = wave_d[0];
    for (int w = 1; w < (nt >> 6); ++w)
      if (better(wave_q[w], wave_d[w], bq, bd)) bq = wave_q[w], bd = wave_d[w];
    d_prev = bd;  // the same in every thread; the next seam's barrier orders these reads before its winners' writes
    if (tid == 0) {
      shift[b] = d_prev;
      if (shift_out) shift_out[b] = d_prev;
    }
  }
}

// out[out_off[b] + j] for j < body[b]. Block (b, blk) takes body samples [blk * kSpan, min(.. + kSpan, body[b])) of
// chunk b and streams them in 16-byte chunks that start on 16-byte boundaries of `out` (a body may start at any 4-byte
// boundary: the first and last chunk of a span are partial and stored sample by sample, so nothing outside the body is
// written). The first X samples of a joined chunk are the crossfade from the predecessor's continuation.
__global__ __launch_bounds__(kWriteThreads) void stitch_write_kernel(const StitchChunk* __restrict__ ch,
                                                                     const int32_t* __restrict__ shift, int X,
                                                                     int blocks_per_chunk, float* __restrict__ out) {
  const int b = blockIdx.x / blocks_per_chunk;
  const int blk = blockIdx.x - b * blocks_per_chunk;
  const int64_t body = ch[b].body;
  const int64_t s0 = (int64_t)blk * kSpan;
  if (s0 >= body) return;
  const int64_t s1 = s0 + kSpan < body ? s0 + kSpan : body;
  const float* row = ch[b].row;
  const int64_t n = ch[b].n;
  const int64_t base = ch[b].lead + shift[b];  // the row index of body sample 0
  float* o = out + ch[b].out_off;
  const float* pa = nullptr;  // the predecessor's continuation, where this block crossfades
  if (ch[b].joined && s0 < X) pa = ch[b - 1].row + (ch[b - 1].lead + shift[b - 1] + ch[b - 1].body);
  const int off = (int)((reinterpret_cast<uintptr_t>(o + s0) >> 2) & 3);
  for (int q = threadIdx.x; q <= kSpan / 4; q += kWriteThreads) {
    const int64_t j0 = s0 - off + 4 * (int64_t)q;  // < s0 in the span's first chunk
    if (j0 >= s1) break;
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool whole = j0 >= s0 && j0 + 4 <= s1;
    if (whole) {
      load4(row, base + j0, n, x);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k >= s0 && j0 + k < s1) x[k] = row[base + j0 + k];
    }
    if (pa && j0 < X) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t j = j0 + k;
        if (j >= s0 && j < s1 && j < X) {
          const double a = (double)pa[j];
          const double w = ((double)j + 0.5) / (double)X;
          x[k] = (float)(a + w * ((double)x[k] - a));
        }
      }
    }
    if (whole) {
      *reinterpret_cast<float4*>(o + j0) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k >= s0 && j0 + k < s1) o[j0 + k] = x[k];
    }
  }
}

}  // namespace

// The host half of svc_stitch (stage_features.hip owns the context and its ring): argument checks before any HIP
// call, one staged table [StitchChunk x B | int32 first chunk of each song x B] with the displacements int32 [B] behind
// it in the same slot, then the two launches. `ring` and `device` point into the context and are read only after the
// checks.
int stitch(StageRing* ring, const int* device, const float* const* rows, int B, const int64_t* n, const int64_t* lead,
           const int64_t* body, const int32_t* joined, const int64_t* out_off, int xfade, int search, double eps,
           float* out, int64_t out_len, int32_t* shift_out, double* q_out, hipStream_t s) {
  SVC_REQUIRE(rows && n && lead && body && joined && out_off, "stitch: null %s table",
              !rows ? "rows" : !n ? "n" : !lead ? "lead" : !body ? "body" : !joined ? "joined" : "out_off");
  SVC_REQUIRE(out, "stitch: null out");
  SVC_REQUIRE(B >= 1, "stitch: B=%d", B);
  SVC_REQUIRE(xfade >= 1 && xfade <= kXfadeMax, "stitch: xfade %d (1..%d)", xfade, kXfadeMax);
  SVC_REQUIRE(search >= 0 && search <= kSearchMax, "stitch: search %d (0..%d)", search, kSearchMax);
  SVC_REQUIRE(eps > 0.0, "stitch: eps %g (must be positive)", eps);
  SVC_REQUIRE(out_len >= 1 && out_len <= kLenMax, "stitch: out_len %lld", (long long)out_len);
  SVC_REQUIRE(joined[0] == 0, "stitch: chunk 0 is joined to a predecessor it does not have");
  const int64_t X = xfade, R = search;
  std::vector<char> buf((size_t)B * sizeof(StitchChunk) + (size_t)B * 4, 0);
  StitchChunk* hc = reinterpret_cast<StitchChunk*>(buf.data());
  int32_t* hfirst = reinterpret_cast<int32_t*>(buf.data() + (size_t)B * sizeof(StitchChunk));
  int songs = 0, seams = 0;
  int64_t max_body = 0;
  double total = 0.0;
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)out_len * 4;
  for (int b = 0; b < B; ++b) {
    SVC_REQUIRE(rows[b], "stitch: chunk %d: null row", b);
    SVC_REQUIRE(joined[b] == 0 || joined[b] == 1, "stitch: chunk %d: joined %d (0 or 1)", b, joined[b]);
    SVC_REQUIRE(n[b] >= 1 && n[b] <= kLenMax, "stitch: chunk %d: %lld usable samples", b, (long long)n[b]);
    SVC_REQUIRE(body[b] >= 1, "stitch: chunk %d: body of %lld samples", b, (long long)body[b]);
    SVC_REQUIRE(out_off[b] >= 0 && out_off[b] <= out_len && body[b] <= out_len - out_off[b],
                "stitch: chunk %d: output interval [%lld, +%lld) outside [0, %lld)", b, (long long)out_off[b],
                (long long)body[b], (long long)out_len);
    if (joined[b]) {
      SVC_REQUIRE(out_off[b] == out_off[b - 1] + body[b - 1],
                  "stitch: chunk %d is joined but its output starts at %lld, its predecessor's ends at %lld", b,
                  (long long)out_off[b], (long long)(out_off[b - 1] + body[b - 1]));
      SVC_REQUIRE(body[b] >= X, "stitch: chunk %d is joined with a body of %lld samples, shorter than xfade %d", b,
                  (long long)body[b], xfade);
    }
    // every row index the definitions read, for any displacement of this chunk and of its predecessor
    const int64_t d_lo = joined[b] ? -R : 0, d_hi = joined[b] && R > 0 ? R - 1 : 0;
    const int64_t tail = b + 1 < B && joined[b + 1] ? X : 0;  // read as the successor's predecessor
    SVC_REQUIRE(lead[b] >= 0 && lead[b] <= n[b] && body[b] <= n[b] && lead[b] + d_lo >= 0 &&
                    lead[b] + d_hi + body[b] + tail <= n[b],
                "stitch: chunk %d: rows [%lld, %lld) are read, the row has [0, %lld)", b, (long long)(lead[b] + d_lo),
                (long long)(lead[b] + d_hi + body[b] + tail), (long long)n[b]);
    const uintptr_t r0 = reinterpret_cast<uintptr_t>(rows[b]), r1 = r0 + (uintptr_t)n[b] * 4;
    SVC_REQUIRE(r1 <= o0 || o1 <= r0, "stitch: chunk %d: out overlaps its row", b);
    hc[b] = StitchChunk{rows[b], n[b], lead[b], body[b], out_off[b], joined[b], 0};
    if (!joined[b]) hfirst[songs++] = b;
    else ++seams;
    max_body = std::max(max_body, body[b]);
    total += (double)body[b];
  }
  {  // no two output intervals share a sample
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return out_off[x] < out_off[y]; });
    for (int i = 0; i + 1 < B; ++i)
      SVC_REQUIRE(out_off[order[i]] + body[order[i]] <= out_off[order[i + 1]],
                  "stitch: the output intervals of chunks %d and %d overlap", order[i], order[i + 1]);
  }
  const int nc = search > 0 ? 2 * search : 1;
  const int64_t bpc = cdiv64(max_body, kSpan);
  SVC_REQUIRE(bpc * B < (1ll << 31), "stitch: %d chunks of up to %lld samples: too large", B, (long long)max_body);
  const int lds = (((xfade + 3) & ~3) + xfade + nc - 1) * 4;

  SVC_HIP_CHECK(hipSetDevice(*device));
  if (lds > 64 * 1024)
    if (int st = ensure_dyn_lds(reinterpret_cast<const void*>(stitch_seams_kernel), lds)) return st;
  RingRetire retire_(*ring, s);
  void* dev = nullptr;
  if (int st = ring->put(buf.data(), buf.size(), s, &dev, (size_t)B * 4)) return st;
  const StitchChunk* d_ch = reinterpret_cast<const StitchChunk*>(dev);
  const int32_t* d_first = reinterpret_cast<const int32_t*>(reinterpret_cast<char*>(dev) + (size_t)B * sizeof(StitchChunk));
  int32_t* d_shift = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(dev) + buf.size());
  {
    const int nt = (int)std::min<int64_t>(kSeamThreads, std::max<int64_t>(256, round_up(nc, 64)));
    const int tok = prof_begin("stitch_seams", 4.0 * seams * (double)nc * (double)xfade,
                               (double)seams * (2.0 * xfade + nc) * 4.0, s);
    hipLaunchKernelGGL(stitch_seams_kernel, dim3((unsigned)songs), dim3(nt), (size_t)lds, s, d_ch, d_first, B, xfade,
                       search, eps, d_shift, shift_out, q_out);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  const int tok = prof_begin("stitch_write", 0.0, total * 8.0, s);
  hipLaunchKernelGGL(stitch_write_kernel, dim3((unsigned)(bpc * B)), dim3(kWriteThreads), 0, s, d_ch, d_shift, xfade,
                     (int)bpc, out);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

}  // namespace svc
