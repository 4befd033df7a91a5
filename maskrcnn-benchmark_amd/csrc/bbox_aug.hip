// bbox_aug.hip — the merge of test-time box augmentation (include/detops.h: detops_bbox_aug_merge_count / _write).
//
// Every (image, augmentation) group hands in its unfiltered per-class boxes [rows, 4C] and scores [rows, C].  The merge
// maps each group's boxes back to the frame of the image's first pass (clamp, un-flip, scale: the reference's BoxList
// arithmetic, engine/bbox_aug.py + structures/bounding_box.py) and compacts the (row, class) pairs above the score
// threshold into one NMS segment per (image, class), in row order — rows are image-major with the passes in order, so row
// order IS "pass order, then row order".
//
// Four launches, no atomics: the order comes from prefix sums only, so two runs write identical bytes.
//   count    a workgroup owns kTileRows rows of one image and one tile of columns; a wave walks kWaveRows of them.  Lanes
//            cover (row, class) pairs with the class the fast index (scores is class-minor: a wave reads consecutive
//            classes of a row, and with few classes several rows at once).  All of a lane's loads are issued before the
//            first ballot (the lane split is a template parameter, so the walk unrolls); per step one ballot, the lanes of
//            one class pick their bits out of it.  -> cnt[image][class][tile, wave]
//   prefix   a wave per (image, class) segment: exclusive prefix over its (tile, wave) counts, in place, and its length
//   offsets  one workgroup: a fixed-shape scan over the segment lengths -> seg_offsets, the total and the longest segment
//   write    the count pass again; position = seg_offsets[segment] + prefix of the (tile, wave) + candidates of the class
//            seen so far by the wave + candidates of the class on lower lanes of this step
#include "detops_dtype.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kWaveRows = 32;                       // rows a wave walks (>= the rows one step of the widest split takes)
constexpr int kTileRows = kWaves * kWaveRows;       // rows a workgroup owns
constexpr int kScanBlock = 1024;

// bit l is set where l % (1 << k) == 0: the lanes that share lane 0's class when a step holds 64 >> k rows
__device__ __constant__ const detops_u64 kEvery[7] = {~0ull, 0x5555555555555555ull, 0x1111111111111111ull, 0x0101010101010101ull,
                                                      0x0001000100010001ull, 0x0000000100000001ull, 1ull};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// torch.clamp(min=0, max=hi): a NaN stays a NaN
__device__ __forceinline__ float clampf(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

// The walk of one lane.  CWL: log2 of the lanes a row takes (the classes of a column tile); a step covers 64 >> CWL rows.
template <int CWL>
struct Walk {
  static constexpr int kRowsPerStep = kWave >> CWL;
  static constexpr int kSteps = kWaveRows / kRowsPerStep;
  int col, sub, lane, r0, r_hi, slot;
  bool live;
  detops_u64 colmask;
  float score[kSteps];

  // the lane's place in workgroup (tile, column tile, image), and its scores: every load in flight before the first use
  __device__ __forceinline__ Walk(const float* __restrict__ scores, const int32_t* __restrict__ row_offset, int R, int C, int T,
                                  float thresh) {
    const int n = blockIdx.z, w = threadIdx.x / kWave;
    lane = threadIdx.x % kWave;
    const int c = lane & ((1 << CWL) - 1);
    col = (blockIdx.y << CWL) + c;
    sub = lane >> CWL;
    colmask = kEvery[CWL] << c;
    live = col >= 1 && col < C;
    const int r_lo = clampi(row_offset[static_cast<int64_t>(n) * T], 0, R);
    r_hi = clampi(row_offset[static_cast<int64_t>(n + 1) * T], r_lo, R);
    r0 = r_lo + blockIdx.x * kTileRows + w * kWaveRows;
    slot = blockIdx.x * kWaves + w;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int r = r0 + s * kRowsPerStep + sub;
      score[s] = (live && r < r_hi) ? scores[static_cast<int64_t>(r) * C + col] : thresh;   // thresh > thresh: no candidate
    }
  }
};

// cnt[image][class][tile * kWaves + wave]: the counts of a segment are contiguous
__device__ __forceinline__ int64_t cnt_index(int C, int per, int col, int slot) {
  return (static_cast<int64_t>(blockIdx.z) * C + col) * per + slot;
}

template <int CWL>
__global__ void __launch_bounds__(kBlock) bbox_aug_count_kernel(const float* __restrict__ scores, const int32_t* __restrict__ row_offset,
                                                                int R, int C, int T, int per, float thresh,
                                                                int32_t* __restrict__ cnt) {
  const Walk<CWL> k(scores, row_offset, R, C, T, thresh);
  int c = 0;
#pragma unroll
  for (int s = 0; s < Walk<CWL>::kSteps; ++s) c += __popcll(__ballot(k.score[s] > thresh) & k.colmask);
  if (k.sub == 0 && k.col < C) cnt[cnt_index(C, per, k.col, k.slot)] = c;
}

// a wave per segment: cnt[segment][0 .. per) -> its exclusive prefix, in place; seg_len[segment] = the sum
__global__ void __launch_bounds__(kBlock) bbox_aug_prefix_kernel(int32_t* __restrict__ cnt, int S, int C, int per,
                                                                 int32_t* __restrict__ seg_len) {
  const int s = blockIdx.x * kWaves + threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (s >= S) return;                                  // wave-uniform
  const int n = s / (C - 1), j = 1 + s % (C - 1);
  int32_t* p = cnt + (static_cast<int64_t>(n) * C + j) * per;
  const int len = scan_tiles<kWave>(per, [&](int i) { return p[i]; }, [&](int i, int before) { p[i] = before; });
  if (lane == 0) seg_len[s] = len;
}

__global__ void __launch_bounds__(kScanBlock) bbox_aug_offsets_kernel(const int32_t* __restrict__ seg_len, int S,
                                                                      int32_t* __restrict__ seg_offsets, int32_t* __restrict__ totals) {
  __shared__ int wave_sums[kScanBlock / kWave];
  int longest = 0;
  const int carry = scan_tiles<kScanBlock>(
      S,
      [&](int s) {
        const int len = seg_len[s];
        longest = len > longest ? len : longest;
        return len;
      },
      [&](int s, int before) { seg_offsets[s] = before; }, wave_sums);
  // the longest segment: a max over the workgroup through the scan's scratch (free again: scan_tiles ends on a barrier)
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    const int u = __shfl_down(longest, d);
    longest = u > longest ? u : longest;
  }
  if (threadIdx.x % kWave == 0) wave_sums[threadIdx.x / kWave] = longest;
  __syncthreads();
  if (threadIdx.x == 0) {
    int m = 0;
    for (int i = 0; i < kScanBlock / kWave; ++i) m = wave_sums[i] > m ? wave_sums[i] : m;
    seg_offsets[S] = carry;
    totals[0] = carry;
    totals[1] = m;
  }
}

template <int CWL>
__global__ void __launch_bounds__(kBlock) bbox_aug_write_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                const int32_t* __restrict__ row_offset,
                                                                const int32_t* __restrict__ group_geom,
                                                                const float* __restrict__ group_ratio, int R, int C, int T, int per,
                                                                float thresh, const int32_t* __restrict__ seg_offsets,
                                                                const int32_t* __restrict__ cnt, int64_t capacity,
                                                                float* __restrict__ cand_boxes, float* __restrict__ cand_scores) {
#pragma clang fp contract(off)
  const Walk<CWL> k(scores, row_offset, R, C, T, thresh);
  const int n = blockIdx.z;
  int64_t run = 0;
  if (k.live) run = static_cast<int64_t>(seg_offsets[static_cast<int64_t>(n) * (C - 1) + k.col - 1]) + cnt[cnt_index(C, per, k.col, k.slot)];
  const detops_u64 below = (1ull << k.lane) - 1ull;
#pragma unroll
  for (int s = 0; s < Walk<CWL>::kSteps; ++s) {
    const float sc = k.score[s];
    const bool pass = sc > thresh;
    const detops_u64 m = __ballot(pass) & k.colmask;
    const int64_t pos = run + __popcll(m & below);
    run += __popcll(m);
    if (!pass || pos < 0 || pos >= capacity) continue;   // the ballot above is the iteration's only wave-wide step
    const int r = k.r0 + s * Walk<CWL>::kRowsPerStep + k.sub;
    int t = 0;                                         // the row's pass: the groups of image n are consecutive
    while (t < T - 1 && r >= row_offset[static_cast<int64_t>(n) * T + t + 1]) ++t;
    const int64_t g = static_cast<int64_t>(n) * T + t;
    const float fw = static_cast<float>(group_geom[g * 3 + 0]), xhi = static_cast<float>(group_geom[g * 3 + 0] - 1);
    const float yhi = static_cast<float>(group_geom[g * 3 + 1] - 1);
    const float4 b = *reinterpret_cast<const float4*>(boxes + (static_cast<int64_t>(r) * C + k.col) * 4);
    float x1 = clampf(b.x, xhi), y1 = clampf(b.y, yhi), x2 = clampf(b.z, xhi), y2 = clampf(b.w, yhi);
    if (group_geom[g * 3 + 2] & 1) {                   // BoxList.transpose(FLIP_LEFT_RIGHT): width - xmax - 1, width - xmin - 1
      const float fx1 = (fw - x2) - 1.f, fx2 = (fw - x1) - 1.f;
      x1 = fx1;
      x2 = fx2;
    }
    if (t > 0) {                                       // BoxList.resize to the first pass's frame: one multiply each
      const float rx = group_ratio[g * 2 + 0], ry = group_ratio[g * 2 + 1];
      x1 = x1 * rx;
      y1 = y1 * ry;
      x2 = x2 * rx;
      y2 = y2 * ry;
    }
    *reinterpret_cast<float4*>(cand_boxes + pos * 4) = make_float4(x1, y1, x2, y2);
    cand_scores[pos] = sc;
  }
}

// lanes per row: the smallest power of two that holds C; beyond 32 classes, 32 or 64 lanes per column tile, whichever
// leaves fewer idle lanes over the tiles (C = 81: three tiles of 32, 81 of 96 lanes live, where two of 64 have 81 of 128)
int lane_split_log2(int C) {
  int k = 1;
  while ((1 << k) < C && k < 5) ++k;
  if (C <= 32) return k;
  const int pad32 = (C + 31) / 32 * 32, pad64 = (C + 63) / 64 * 64;
  return pad32 < pad64 ? 5 : 6;
}

// rows of the longest image and a check of the host copy of row_offset; < 0: malformed
int64_t longest_image(const int32_t* row_offset_host, int R, int N, int T) {
  const int64_t G = static_cast<int64_t>(N) * T;
  if (row_offset_host[0] != 0 || row_offset_host[G] != R) return -1;
  for (int64_t g = 0; g < G; ++g)
    if (row_offset_host[g + 1] < row_offset_host[g]) return -1;
  int64_t longest = 0;
  for (int n = 0; n < N; ++n) {
    const int64_t rows = row_offset_host[static_cast<int64_t>(n + 1) * T] - row_offset_host[static_cast<int64_t>(n) * T];
    longest = rows > longest ? rows : longest;
  }
  return longest;
}

struct Shape {
  int tiles, per, col_tiles, cw_log2, S;
  size_t cnt_bytes, bytes;       // the counts, then the segment lengths
};

bool shape_ok(int R, int C, int N, int T) {
  return R >= 0 && C >= 1 && N >= 0 && T >= 1 && N <= 65535 && static_cast<int64_t>(N) * T < (1ll << 30) &&
         static_cast<int64_t>(R) * C <= 0x7fffffffll && static_cast<int64_t>(N) * C <= 0x7fffffffll;
}

Shape make_shape(int N, int C, int64_t max_image_rows) {
  Shape s;
  s.tiles = static_cast<int>(ceil_div64(max_image_rows, kTileRows));
  s.per = s.tiles * kWaves;
  s.cw_log2 = lane_split_log2(C);
  s.col_tiles = (C + (1 << s.cw_log2) - 1) >> s.cw_log2;
  s.S = N * (C - 1);
  s.cnt_bytes = (static_cast<size_t>(N) * C * s.per * sizeof(int32_t) + 15) / 16 * 16;
  s.bytes = s.cnt_bytes + static_cast<size_t>(s.S) * sizeof(int32_t);
  return s;
}

// the kernel of a lane split
#define BBOX_AUG_DISPATCH(cw_log2, LAUNCH)                         \
  switch (cw_log2) {                                               \
    case 1: LAUNCH(1); break;                                      \
    case 2: LAUNCH(2); break;                                      \
    case 3: LAUNCH(3); break;                                      \
    case 4: LAUNCH(4); break;                                      \
    case 5: LAUNCH(5); break;                                      \
    default: LAUNCH(6); break;                                     \
  }

}  // namespace

DETOPS_API size_t detops_bbox_aug_merge_workspace_bytes(int N, int C, int max_image_rows) {
  if (N < 0 || C < 1 || max_image_rows < 0) return 0;
  return make_shape(N, C, max_image_rows).bytes + 16;
}

DETOPS_API int detops_bbox_aug_merge_count(const float* scores, const int32_t* row_offset, const int32_t* row_offset_host, int R,
                                           int C, int N, int T, float score_thresh, int32_t* seg_offsets, int32_t* totals,
                                           void* workspace, size_t workspace_bytes, detops_stream_t stream) {
  if (!shape_ok(R, C, N, T) || !seg_offsets || !totals) return DETOPS_EINVAL;
  Shape s = make_shape(N, C, 0);
  if (s.S > 0) {
    if (!row_offset || !row_offset_host || !workspace) return DETOPS_EINVAL;
    const int64_t longest = longest_image(row_offset_host, R, N, T);
    if (longest < 0) return DETOPS_EINVAL;
    s = make_shape(N, C, longest);
    if (s.tiles > 0 && !scores) return DETOPS_EINVAL;
    if (workspace_bytes < s.bytes) return DETOPS_EWORKSPACE;
    if (s.col_tiles > 65535) return DETOPS_EINVAL;
  }
  int32_t* cnt = static_cast<int32_t*>(workspace);
  int32_t* seg_len = s.S > 0 ? reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + s.cnt_bytes) : nullptr;
  if (s.S > 0 && s.tiles > 0) {
#define LAUNCH(K)                                                                                                             \
  hipLaunchKernelGGL(bbox_aug_count_kernel<K>, dim3(s.tiles, s.col_tiles, N), dim3(kBlock), 0, as_stream(stream), scores, \
                     row_offset, R, C, T, s.per, score_thresh, cnt)
    BBOX_AUG_DISPATCH(s.cw_log2, LAUNCH)
#undef LAUNCH
    const int rc = launch_status();
    if (rc) return rc;
  }
  if (s.S > 0) {                                       // (per == 0: every length is written as 0)
    hipLaunchKernelGGL(bbox_aug_prefix_kernel, dim3((s.S + kWaves - 1) / kWaves), dim3(kBlock), 0, as_stream(stream), cnt, s.S, C,
                       s.per, seg_len);
    const int rc = launch_status();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(bbox_aug_offsets_kernel, dim3(1), dim3(kScanBlock), 0, as_stream(stream), seg_len, s.S, seg_offsets, totals);
  return launch_status();
}

DETOPS_API int detops_bbox_aug_merge_write(const float* boxes, const float* scores, const int32_t* row_offset,
                                           const int32_t* row_offset_host, const int32_t* group_geom, const float* group_ratio,
                                           int R, int C, int N, int T, float score_thresh, const int32_t* seg_offsets,
                                           int64_t capacity, float* cand_boxes, float* cand_scores, const void* workspace,
                                           size_t workspace_bytes, detops_stream_t stream) {
  if (!shape_ok(R, C, N, T) || capacity < 0) return DETOPS_EINVAL;
  if (N == 0 || C < 2 || R == 0 || capacity == 0) return 0;
  if (!boxes || !scores || !row_offset || !row_offset_host || !group_geom || !group_ratio || !seg_offsets || !cand_boxes ||
      !cand_scores || !workspace)
    return DETOPS_EINVAL;
  if (reinterpret_cast<uintptr_t>(boxes) % 16 || reinterpret_cast<uintptr_t>(cand_boxes) % 16) return DETOPS_EINVAL;   // float4 access
  const int64_t longest = longest_image(row_offset_host, R, N, T);
  if (longest < 0) return DETOPS_EINVAL;
  const Shape s = make_shape(N, C, longest);
  if (s.col_tiles > 65535) return DETOPS_EINVAL;
  if (workspace_bytes < s.bytes) return DETOPS_EWORKSPACE;
  if (s.tiles == 0) return 0;
  const int32_t* cnt = static_cast<const int32_t*>(workspace);
#define LAUNCH(K)                                                                                                                 \
  hipLaunchKernelGGL(bbox_aug_write_kernel<K>, dim3(s.tiles, s.col_tiles, N), dim3(kBlock), 0, as_stream(stream), boxes, scores, \
                     row_offset, group_geom, group_ratio, R, C, T, s.per, score_thresh, seg_offsets, cnt, capacity, cand_boxes,   \
                     cand_scores)
  BBOX_AUG_DISPATCH(s.cw_log2, LAUNCH)
#undef LAUNCH
  return launch_status();
}
