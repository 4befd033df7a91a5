// eval_proposals.hip — the greedy matching behind the average recall of RPN proposals, for gfx950 (MI355X).  The rules are
// stated in include/detops.h ("Proposal recall"); maskrcnn_benchmark/_eval_cpu.py (eval_proposal_overlaps) is the same in
// numpy, written as the reference's loop.
//
//   detops_eval_proposal_overlaps   sorted proposals and ground truths of a batch -> per (limit, area range) the IoU every
//                                   ground truth is matched with (0: not reached, -1: outside the range)
//
// One workgroup per (image, limit, area range).  The image's boxes are staged in LDS once; the [P, G] IoU matrix never
// exists.  Every ground truth (a "column") keeps its best (IoU, proposal) among the proposals not yet retired.  A round is
//   - an argmax over the open columns (a thread per column, a shuffle tree per wave, the waves' results through LDS);
//   - the winner's column and proposal are retired;
//   - only the columns whose best WAS the retired proposal are scanned again: a wave per column, a lane per proposal.
// The first round's scan is the same code: every column starts with "best = proposal -1" and "the retired proposal" starts
// at -1.  Ties go to the lowest index at every level (a thread walks its indices upwards and replaces on `>` only; two
// candidates of equal value keep the lower index), which is the first maximum the reference's torch.max returns.
// Column g is scanned by wave g % kWaves, so a few ground truths still keep all waves busy.  A candidate is made only by
// `v > best`, starting from -inf: a NaN IoU is never a candidate, and an index is always one a loop ran over.
// Two barriers a round, no atomics, every output element written exactly once at the end.
#include "detops_dtype.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxDt = DETOPS_EVAL_PROPOSALS_MAX_DT;
constexpr int kMaxGt = DETOPS_EVAL_PROPOSALS_MAX_GT;
constexpr unsigned char kOff = 0, kOpen = 1, kDone = 2;     // a column: outside the area range | not matched yet | matched

struct Best {
  float v;
  int i;            // the index that attains v; < 0: no candidate
};

__device__ __forceinline__ Best no_candidate() {
  Best b;
  b.v = -__builtin_huge_valf();
  b.i = -1;
  return b;
}

// the larger value; of equal values the lower index; no candidate loses
__device__ __forceinline__ Best better(Best a, Best b) {
  const bool take = b.i >= 0 && (a.i < 0 || b.v > a.v || (b.v == a.v && b.i < a.i));
  return take ? b : a;
}

// over the wave, valid in lane 0
__device__ __forceinline__ Best wave_best(Best x) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    Best o;
    o.v = __shfl_down(x.v, off);
    o.i = __shfl_down(x.i, off);
    x = better(x, o);
  }
  return x;
}

__device__ __forceinline__ float box_area(float4 b) {
#pragma clang fp contract(off)
  float w = b.z - b.x; w = w + 1.0f;
  float h = b.w - b.y; h = h + 1.0f;
  return w * h;
}

// boxlist_iou of a proposal and a ground truth (whose area the caller holds)
__device__ __forceinline__ float proposal_iou(float4 p, float4 g, float area_g) {
#pragma clang fp contract(off)
  const float area_p = box_area(p);
  float w = fminf(p.z, g.z) - fmaxf(p.x, g.x); w = w + 1.0f; w = fmaxf(w, 0.0f);
  float h = fminf(p.w, g.w) - fmaxf(p.y, g.y); h = h + 1.0f; h = fmaxf(h, 0.0f);
  const float inter = w * h;
  float u = area_p + area_g;
  u = u - inter;
  return inter / u;
}

__device__ __forceinline__ float4 load_box(const float* __restrict__ boxes, int64_t i) {
  const float* b = boxes + 4 * i;
  return make_float4(b[0], b[1], b[2], b[3]);
}

// the LDS of a workgroup, every part a multiple of 16 bytes (dt_cap and gt_cap are multiples of 16)
__host__ __device__ __forceinline__ size_t lds_bytes(int dt_cap, int gt_cap) {
  return static_cast<size_t>(dt_cap) * 17 + static_cast<size_t>(gt_cap) * 25 + kWaves * sizeof(Best);
}
static inline int round16(int n) { return n < 16 ? 16 : (n + 15) / 16 * 16; }

__global__ void __launch_bounds__(kBlock)
eval_proposal_overlaps_kernel(const float* __restrict__ dt_boxes, const float* __restrict__ gt_boxes,
                              const int32_t* __restrict__ dt_offset, const int32_t* __restrict__ gt_offset,
                              const unsigned char* __restrict__ gt_valid, const int32_t* __restrict__ limits, int L, int A,
                              int64_t D_total, int64_t G_total, int max_dt, int max_gt, int dt_cap, int gt_cap,
                              float* __restrict__ overlaps) {
  DETOPS_DYNAMIC_LDS(unsigned char, lds);
  float4* dt = reinterpret_cast<float4*>(lds);                  // [dt_cap] the proposals that take part
  float4* gt = dt + dt_cap;                                     // [gt_cap]
  float* col_v = reinterpret_cast<float*>(gt + gt_cap);         // [gt_cap] a column's best IoU among the unused proposals;
  int* col_p = reinterpret_cast<int*>(col_v + gt_cap);          // [gt_cap] ... and the proposal (-1: none).  Matched: the result
  Best* red = reinterpret_cast<Best*>(col_p + gt_cap);          // [kWaves]
  unsigned char* state = reinterpret_cast<unsigned char*>(red + kWaves);   // [gt_cap] kOff | kOpen | kDone
  unsigned char* used = state + gt_cap;                         // [dt_cap] the proposal is retired

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int a = blockIdx.x % A, l = (blockIdx.x / A) % L, n = blockIdx.x / (A * L);
  const int d0 = dt_offset[n], g0 = gt_offset[n];
  int P = dt_offset[n + 1] - d0;
  const int G = gt_offset[n + 1] - g0;
  // (uniform over the workgroup) an image without ground truth has no slot to write; offsets that leave the arrays: nothing
  if (G <= 0 || P < 0 || d0 < 0 || g0 < 0 || static_cast<int64_t>(d0) + P > D_total || static_cast<int64_t>(g0) + G > G_total)
    return;
  const int lim = limits[l];
  if (lim > 0 && P > lim) P = lim;
  if (P > max_dt) P = max_dt;
  const int Gs = G < max_gt ? G : max_gt;                       // the columns that are matched
  const unsigned char* valid = gt_valid + static_cast<int64_t>(a) * G_total + g0;
  float* out = overlaps + (static_cast<int64_t>(l) * A + a) * G_total + g0;

  for (int p = tid; p < P; p += kBlock) {
    dt[p] = load_box(dt_boxes, static_cast<int64_t>(d0) + p);
    used[p] = 0;
  }
  for (int g = tid; g < Gs; g += kBlock) {
    gt[g] = load_box(gt_boxes, static_cast<int64_t>(g0) + g);
    state[g] = valid[g] ? kOpen : kOff;
    col_v[g] = 0.0f;
    col_p[g] = -1;
  }
  for (int g = Gs + tid; g < G; g += kBlock) out[g] = valid[g] ? 0.0f : -1.0f;      // (beyond the stated max_gt)
  __syncthreads();

  const int rounds = P < Gs ? P : Gs;
  int sel_p = -1, sel_g = -1;           // what the round before retired (thread 0 is still writing the two flags)
  for (int r = 0; r < rounds; ++r) {
    // columns that lost their best proposal (first round: all open ones): wave `wave` owns the columns g % kWaves == wave
    for (int jb = 0; wave + kWaves * jb < Gs; jb += kWave) {
      const int g = wave + kWaves * (jb + lane);
      const bool need = g < Gs && g != sel_g && state[g] == kOpen && col_p[g] == sel_p;
      detops_u64 todo = __ballot(need);
      while (todo) {                                            // (uniform over the wave)
        const int c = wave + kWaves * (jb + __builtin_ctzll(todo));
        todo &= todo - 1;
        const float4 gb = gt[c];
        const float area_g = box_area(gb);
        Best b = no_candidate();
        for (int p = lane; p < P; p += kWave) {
          if (p == sel_p || used[p]) continue;
          const float v = proposal_iou(dt[p], gb, area_g);
          if (v > b.v) { b.v = v; b.i = p; }
        }
        b = wave_best(b);
        if (lane == 0) { col_v[c] = b.v; col_p[c] = b.i; }
      }
    }
    __syncthreads();
    // the open column with the largest best
    Best b = no_candidate();
    for (int g = tid; g < Gs; g += kBlock) {
      if (state[g] != kOpen || col_p[g] < 0) continue;
      const float v = col_v[g];
      if (v > b.v) { b.v = v; b.i = g; }
    }
    b = wave_best(b);
    if (lane == 0) red[wave] = b;
    __syncthreads();
    b = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) b = better(b, red[w]);
    if (b.i < 0) break;                                         // (uniform) no open column has an unused proposal left
    sel_g = b.i;
    sel_p = col_p[sel_g];
    // col_v[sel_g] stays: it is the recorded overlap.  Nobody reads these two flags before the next barrier: the scan
    // above skips sel_g and sel_p by value.
    if (tid == 0) { state[sel_g] = kDone; used[sel_p] = 1; }
  }
  __syncthreads();
  for (int g = tid; g < Gs; g += kBlock) {
    const unsigned char s = state[g];
    out[g] = s == kOff ? -1.0f : (s == kDone ? col_v[g] : 0.0f);
  }
}

}  // namespace

DETOPS_API int detops_eval_proposal_overlaps(const float* dt_boxes, const float* gt_boxes, const int32_t* dt_offset,
                                             const int32_t* gt_offset, const unsigned char* gt_valid, const int32_t* limits,
                                             int N, int L, int A, int64_t D_total, int64_t G_total, int max_dt, int max_gt,
                                             float* overlaps, detops_stream_t stream) {
  if (N < 0 || L < 1 || A < 1 || D_total < 0 || G_total < 0 || max_dt < 0 || max_gt < 0) return DETOPS_EINVAL;
  if (static_cast<int64_t>(N) * L * A > 0x7fffffff) return DETOPS_EINVAL;
  if (N == 0 || G_total == 0) return 0;
  if (!dt_offset || !gt_offset || !gt_boxes || !gt_valid || !limits || !overlaps || (D_total > 0 && !dt_boxes))
    return DETOPS_EINVAL;
  if (max_dt > kMaxDt || max_gt > kMaxGt) return DETOPS_EUNSUPPORTED;
  const int dt_cap = round16(max_dt), gt_cap = round16(max_gt);
  static_assert(static_cast<size_t>(kMaxDt) * 17 + static_cast<size_t>(kMaxGt) * 25 + kWaves * sizeof(Best) <= 64 * 1024,
                "the default dynamic LDS limit; two workgroups per CU at the caps");
  hipLaunchKernelGGL(eval_proposal_overlaps_kernel, dim3(static_cast<unsigned>(N * L * A)), dim3(kBlock),
                     lds_bytes(dt_cap, gt_cap), as_stream(stream), dt_boxes, gt_boxes, dt_offset, gt_offset, gt_valid, limits,
                     L, A, D_total, G_total, max_dt, max_gt, dt_cap, gt_cap, overlaps);
  return launch_status();
}
