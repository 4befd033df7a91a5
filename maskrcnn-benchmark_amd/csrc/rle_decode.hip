// rle_decode.hip — COCO's compressed RLE strings back to uncompressed runs, for gfx950 (MI355X): the inverse of
// rle_string.hip.  The decoding is defined in include/detops.h, "Reading compressed RLE strings".
//
//   detops_rle_decode_count   values of every chunk of the flat byte array, one scan over the chunks, the run offset of
//                             every mask; [one host read of the total: run_offset[N]]
//   detops_rle_decode_write   the runs and the per-mask status
//
// The work is cut by chunks of kChunk bytes of the FLAT array, never by mask: one string has 50,000 values and its
// neighbour three.  A thread owns kPer consecutive bytes; a byte finds its mask by a binary search in byte_offset for the
// thread's first byte and a walk from there.  A value belongs to the thread of its LAST byte, which walks back at most 6
// bytes.  The two interleaved running sums of a mask (odd runs, even runs from run 2 on) are differences of two PLAIN
// prefix sums over the flat value array — the sum up to the value minus the sum in front of the mask's first value — so
// no scan is segmented; the per-mask status bits are differences of prefix counts in the same way.  Every prefix is a
// block_scan inside a chunk and one scan_tiles over the chunks: a fixed order, no atomics, every output written once.
#include "detops_dtype.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPer = 8;                          // consecutive bytes of a thread
constexpr int kChunk = kBlock * kPer;            // bytes of a workgroup
constexpr int kMaxLen = 7;                       // bytes of a value that is the difference of two int32 values at most
constexpr int kWaves = kBlock / kWave;
constexpr int kStats = 4;                        // per mask: bad bytes, overlong values, runs out of range, sum of the runs

__device__ __forceinline__ int code_of(const uint8_t* __restrict__ bytes, int64_t i) {
  return (static_cast<int>(bytes[i]) - 48) & 0xff;
}

struct ThreadBytes {
  int64_t start[kPer];  // first byte of the byte's mask, clamped to 0
  int code[kPer];       // (byte - 48) & 0xff
  int mask[kPer];
  bool end[kPer];       // last byte of a value: continuation bit clear, or the last byte of its mask
  bool first[kPer];     // first byte of its mask
  bool valid[kPer];     // inside the array
  int ends;
};

__device__ __forceinline__ ThreadBytes load_bytes(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ bo, int N,
                                                  int64_t B, int64_t i0) {
  ThreadBytes r;
  r.ends = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    r.start[j] = 0;
    r.code[j] = 0;
    r.mask[j] = 0;
    r.end[j] = r.first[j] = r.valid[j] = false;
  }
  if (i0 >= B) return r;
  int m = last_at_or_below(bo, N, i0);   // empty strings share their successor's offset: the last one owns i0
  int64_t start = bo[m];
  int64_t next = m + 1 < N ? bo[m + 1] : B;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = i0 + j;
    if (i >= B) break;
    while (i >= next && m + 1 < N) {  // at most N steps, whatever byte_offset holds
      ++m;
      start = next;
      next = m + 1 < N ? bo[m + 1] : B;
    }
    const int c = code_of(bytes, i);
    r.start[j] = start < 0 ? 0 : start;
    r.code[j] = c;
    r.mask[j] = m;
    r.end[j] = !(c & 0x20) || i + 1 == next;
    r.first[j] = i == start;
    r.valid[j] = true;
    r.ends += r.end[j];
  }
  return r;
}

// the value whose last byte is i: its 5-bit groups from the low end, sign-extended from bit 0x10 of the last group.
// Walks back over at most kMaxLen - 1 bytes of the same mask; a value of more bytes is `overlong` and gives the value of
// its last kMaxLen bytes.
__device__ __forceinline__ int64_t value_at(const uint8_t* __restrict__ bytes, int64_t i, int64_t start, int code,
                                            bool& overlong) {
  detops_u64 x = static_cast<detops_u64>(code & 0x1f);
  int len = 1;
  int64_t p = i - 1;
  for (; len < kMaxLen && p >= start; ++len, --p) {
    const int c = code_of(bytes, p);
    if (!(c & 0x20)) break;
    x = (x << 5) | static_cast<detops_u64>(c & 0x1f);
  }
  overlong = len == kMaxLen && p >= start && (code_of(bytes, p) & 0x20);
  if (code & 0x10) x |= ~0ull << (5 * len);
  return static_cast<int64_t>(x);
}

struct ThreadValues {
  int64_t x[kPer];      // the value that ends at the byte
  int cls[kPer];        // 0: no value ends here; 1: run 0 of its mask; 2: an odd run; 3: an even run from run 2 on
  bool overlong[kPer];
  int64_t g;            // flat index of the thread's first value
};

__device__ __forceinline__ ThreadValues load_values(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ ro,
                                                    const ThreadBytes& r, int64_t i0, int64_t g0) {
  ThreadValues v;
  v.g = g0;
  int64_t g = g0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    v.x[j] = 0;
    v.cls[j] = 0;
    v.overlong[j] = false;
    if (!r.end[j]) continue;
    v.x[j] = value_at(bytes, i0 + j, r.start[j], r.code[j], v.overlong[j]);
    const int64_t k = g - ro[r.mask[j]];           // index of the run inside its mask
    v.cls[j] = k == 0 ? 1 : ((k & 1) ? 2 : 3);
    ++g;
  }
  return v;
}

// every mask q whose string starts at byte i (mask m and the empty strings in front of it): f(q)
template <typename F>
__device__ __forceinline__ void for_masks_starting_at(const int64_t* __restrict__ bo, int m, int64_t i, F f) {
  for (int q = m; q >= 0 && bo[q] == i; --q) f(q);
}

// chunk_values[chunk] = values of the chunk; run_offset[m] = values of the chunk in front of mask m's first byte, written
// by the thread that owns that byte
__global__ void __launch_bounds__(kBlock)
rle_decode_count_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ bo, int N, int64_t B,
                        int64_t* __restrict__ chunk_values, int64_t* __restrict__ run_offset) {
  __shared__ int wave_tot[kWaves];
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kPer;
  const ThreadBytes r = load_bytes(bytes, bo, N, B, i0);
  int all;
  int off = block_scan<kBlock>(r.ends, wave_tot, all) - r.ends;
  if (threadIdx.x == 0) chunk_values[blockIdx.x] = all;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (r.first[j]) for_masks_starting_at(bo, r.mask[j], i0 + j, [&](int q) { run_offset[q] = off; });
    off += r.end[j];
  }
}

// the value at entry j of a per-mask table of in-chunk prefixes, made global: the base of the chunk of the mask's first
// byte + what the chunk's kernel left; `all` for a mask that starts at the end of the array
__device__ __forceinline__ int64_t global_prefix(const int64_t* __restrict__ bo, int j, int N, int64_t B,
                                                 const int64_t* __restrict__ chunk_base, int64_t local, int64_t all) {
  const int64_t first = bo[j];
  return (j == N || first >= B || first < 0) ? all : chunk_base[first / kChunk] + local;
}

// One workgroup: chunk_values to its exclusive sum in place, then run_offset[m] made global
__global__ void __launch_bounds__(kBlock)
rle_decode_offsets_kernel(const int64_t* __restrict__ bo, int N, int64_t B, int64_t nchunks,
                          int64_t* __restrict__ chunk_values, int64_t* __restrict__ run_offset) {
  __shared__ int64_t wave_tot[kWaves];
  const int64_t carry = scan_tiles<kBlock>(
      nchunks, [&](int64_t b) { return chunk_values[b]; }, [&](int64_t b, int64_t before) { chunk_values[b] = before; }, wave_tot);
  for (int64_t j = threadIdx.x; j <= N; j += kBlock)
    run_offset[j] = global_prefix(bo, static_cast<int>(j), N, B, chunk_values, run_offset[j], carry);
}

// the thread's bytes and values (both write-phase kernels start with this)
__device__ __forceinline__ ThreadValues decode_thread(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ bo,
                                                      const int64_t* __restrict__ ro, int N, int64_t B,
                                                      const int64_t* __restrict__ chunk_base, int64_t i0, int* wave_tot,
                                                      ThreadBytes& r) {
  r = load_bytes(bytes, bo, N, B, i0);
  int all;
  const int off = block_scan<kBlock>(r.ends, wave_tot, all) - r.ends;
  return load_values(bytes, ro, r, i0, chunk_base[blockIdx.x] + off);
}

// chunk_sum[p][chunk] = sum of the chunk's odd (p = 0) / even (p = 1) runs' values; mask_sum[p][m] = the same sum over the
// values of the chunk in front of mask m's first byte
__global__ void __launch_bounds__(kBlock)
rle_decode_sums_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ bo, const int64_t* __restrict__ ro,
                       int N, int64_t B, const int64_t* __restrict__ chunk_base, int64_t nchunks,
                       int64_t* __restrict__ chunk_sum, int64_t* __restrict__ mask_sum) {
  __shared__ int wave_n[kWaves];
  __shared__ int64_t wave_s[2][kWaves];
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kPer;
  ThreadBytes r;
  const ThreadValues v = decode_thread(bytes, bo, ro, N, B, chunk_base, i0, wave_n, r);
  int64_t odd = 0, even = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (v.cls[j] == 2) odd += v.x[j];
    if (v.cls[j] == 3) even += v.x[j];
  }
  int64_t all_odd, all_even;
  int64_t before_odd = block_scan<kBlock>(odd, wave_s[0], all_odd) - odd;
  int64_t before_even = block_scan<kBlock>(even, wave_s[1], all_even) - even;
  if (threadIdx.x == 0) {
    chunk_sum[blockIdx.x] = all_odd;
    chunk_sum[nchunks + blockIdx.x] = all_even;
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (r.first[j])
      for_masks_starting_at(bo, r.mask[j], i0 + j, [&](int q) {
        mask_sum[q] = before_odd;
        mask_sum[N + q] = before_even;
      });
    if (v.cls[j] == 2) before_odd += v.x[j];
    if (v.cls[j] == 3) before_even += v.x[j];
  }
}

// One workgroup: both rows of chunk_sum to their exclusive sums in place, then mask_sum made global
__global__ void __launch_bounds__(kBlock)
rle_decode_sum_offsets_kernel(const int64_t* __restrict__ bo, int N, int64_t B, int64_t nchunks,
                              int64_t* __restrict__ chunk_sum, int64_t* __restrict__ mask_sum) {
  __shared__ int64_t wave_tot[kWaves];
  for (int p = 0; p < 2; ++p) {
    int64_t* row = chunk_sum + p * nchunks;
    scan_tiles<kBlock>(
        nchunks, [&](int64_t b) { return row[b]; }, [&](int64_t b, int64_t before) { row[b] = before; }, wave_tot);
  }
  for (int64_t j = threadIdx.x; j < N; j += kBlock)
    for (int p = 0; p < 2; ++p)
      mask_sum[p * N + j] = global_prefix(bo, static_cast<int>(j), N, B, chunk_sum + p * nchunks, mask_sum[p * N + j], 0);
}

// The runs: run k > 0 of a mask = (the plain prefix sum of its class up to the value) - (that sum in front of the mask).
// Then the per-mask statistics, as prefixes again: stat_chunk[s][chunk] and stat_local[s][m] (s: bytes outside 48..111,
// overlong values, runs outside [0, 2^31), sum of the runs).
__global__ void __launch_bounds__(kBlock)
rle_decode_write_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ bo, const int64_t* __restrict__ ro,
                        int N, int64_t B, int64_t total, const int64_t* __restrict__ chunk_base, int64_t nchunks,
                        const int64_t* __restrict__ chunk_sum, const int64_t* __restrict__ mask_sum,
                        int32_t* __restrict__ counts, int64_t* __restrict__ stat_chunk, int64_t* __restrict__ stat_local) {
  __shared__ int wave_n[kWaves];
  __shared__ int64_t wave_s[2 + kStats][kWaves];
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kPer;
  ThreadBytes r;
  ThreadValues v = decode_thread(bytes, bo, ro, N, B, chunk_base, i0, wave_n, r);
  int64_t odd = 0, even = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (v.cls[j] == 2) odd += v.x[j];
    if (v.cls[j] == 3) even += v.x[j];
  }
  int64_t unused;
  int64_t run_odd = chunk_sum[blockIdx.x] + block_scan<kBlock>(odd, wave_s[0], unused) - odd;
  int64_t run_even = chunk_sum[nchunks + blockIdx.x] + block_scan<kBlock>(even, wave_s[1], unused) - even;
  int64_t stat[kStats] = {0, 0, 0, 0};
  bool bad_run[kPer];
  int64_t g = v.g;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    bad_run[j] = false;
    if (r.valid[j] && r.code[j] > 63) ++stat[0];
    if (!v.cls[j]) continue;
    int64_t c = v.x[j];
    if (v.cls[j] == 2) c = (run_odd += c) - mask_sum[r.mask[j]];
    if (v.cls[j] == 3) c = (run_even += c) - mask_sum[N + r.mask[j]];
    v.x[j] = c;                                   // from here on: the run
    bad_run[j] = c < 0 || c > INT32_MAX;
    if (g >= 0 && g < total) counts[g] = static_cast<int32_t>(c);
    ++g;
    stat[1] += v.overlong[j];
    stat[2] += bad_run[j];
    stat[3] += c;
  }
  int64_t before[kStats];
#pragma unroll
  for (int s = 0; s < kStats; ++s) {
    int64_t all;
    before[s] = block_scan<kBlock>(stat[s], wave_s[2 + s], all) - stat[s];
    if (threadIdx.x == 0) stat_chunk[s * nchunks + blockIdx.x] = all;
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (r.first[j])
      for_masks_starting_at(bo, r.mask[j], i0 + j, [&](int q) {
#pragma unroll
        for (int s = 0; s < kStats; ++s) stat_local[s * (static_cast<int64_t>(N) + 1) + q] = before[s];
      });
    if (r.valid[j] && r.code[j] > 63) ++before[0];
    if (!v.cls[j]) continue;
    before[1] += v.overlong[j];
    before[2] += bad_run[j];
    before[3] += v.x[j];
  }
}

// One workgroup: the rows of stat_chunk to their exclusive sums in place; then a mask's statistics are the difference of
// the global prefixes at its two ends, and its status the bits of include/detops.h
__global__ void __launch_bounds__(kBlock)
rle_decode_status_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ bo, int N, int64_t B,
                         int64_t nchunks, const int32_t* __restrict__ hw, int64_t* __restrict__ stat_chunk,
                         const int64_t* __restrict__ stat_local, int32_t* __restrict__ status) {
  __shared__ int64_t wave_tot[kWaves];
  int64_t all[kStats];
  for (int s = 0; s < kStats; ++s) {
    int64_t* row = stat_chunk + s * nchunks;
    all[s] = scan_tiles<kBlock>(
        nchunks, [&](int64_t b) { return row[b]; }, [&](int64_t b, int64_t before) { row[b] = before; }, wave_tot);
  }
  const int64_t stride = static_cast<int64_t>(N) + 1;
  for (int64_t j = threadIdx.x; j < N; j += kBlock) {
    int64_t d[kStats];
    for (int s = 0; s < kStats; ++s) {
      const int64_t* row = stat_chunk + s * nchunks;
      const int m = static_cast<int>(j);
      d[s] = global_prefix(bo, m + 1, N, B, row, stat_local[s * stride + j + 1], all[s]) -
             global_prefix(bo, m, N, B, row, stat_local[s * stride + j], all[s]);
    }
    const int64_t b0 = bo[j], b1 = bo[j + 1];
    int st = 0;
    if (d[0]) st |= DETOPS_RLE_BAD_BYTE;
    if (b1 > b0 && b1 >= 1 && b1 <= B && (code_of(bytes, b1 - 1) & 0x20)) st |= DETOPS_RLE_TRUNCATED;
    if (d[1]) st |= DETOPS_RLE_LONG_VALUE;
    if (d[2]) st |= DETOPS_RLE_BAD_RUN;
    if (hw && d[3] != static_cast<int64_t>(hw[2 * j]) * hw[2 * j + 1]) st |= DETOPS_RLE_BAD_SUM;
    status[j] = st;
  }
}

int64_t chunks_of(int64_t B) { return (B + kChunk - 1) / kChunk; }

// 0: launch; 1: nothing to do; < 0: the error
int check_args(int64_t B, int N) {
  if (N < 0 || B < 0) return DETOPS_EINVAL;
  if (N == 0 || B == 0) return 1;
  if (chunks_of(B) > INT32_MAX) return DETOPS_EINVAL;
  return 0;
}

}  // namespace

// int64 elements: chunk bases, 2 rows of chunk sums, kStats rows of chunk statistics; 2 rows of per-mask sums, kStats
// rows of per-mask statistics (N + 1 entries each)
DETOPS_API size_t detops_rle_decode_workspace_bytes(int64_t B, int N) {
  if (B <= 0 || N <= 0) return 0;
  return static_cast<size_t>((3 + kStats) * chunks_of(B) + 2 * static_cast<int64_t>(N) +
                             kStats * (static_cast<int64_t>(N) + 1)) * sizeof(int64_t);
}

DETOPS_API int detops_rle_decode_count(const uint8_t* bytes, const int64_t* byte_offset, int64_t B, int N,
                                       int64_t* run_offset, void* workspace, size_t workspace_bytes,
                                       detops_stream_t stream) {
  const int rc = check_args(B, N);
  if (rc) return rc < 0 ? rc : 0;
  if (!bytes || !byte_offset || !run_offset || !workspace) return DETOPS_EINVAL;
  if (workspace_bytes < detops_rle_decode_workspace_bytes(B, N)) return DETOPS_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const int64_t nchunks = chunks_of(B);
  int64_t* chunk_values = static_cast<int64_t*>(workspace);
  hipLaunchKernelGGL(rle_decode_count_kernel, dim3(static_cast<unsigned>(nchunks)), dim3(kBlock), 0, st, bytes, byte_offset, N,
                     B, chunk_values, run_offset);
  hipLaunchKernelGGL(rle_decode_offsets_kernel, dim3(1), dim3(kBlock), 0, st, byte_offset, N, B, nchunks, chunk_values,
                     run_offset);
  return launch_status();
}

DETOPS_API int detops_rle_decode_write(const uint8_t* bytes, const int64_t* byte_offset, int64_t B, int N,
                                       const int64_t* run_offset, int64_t total, const int32_t* hw, int32_t* counts,
                                       int32_t* status, void* workspace, size_t workspace_bytes, detops_stream_t stream) {
  const int rc = check_args(B, N);
  if (rc) return rc < 0 ? rc : 0;
  if (total < 0 || !bytes || !byte_offset || !run_offset || !status || !workspace || (total > 0 && !counts))
    return DETOPS_EINVAL;
  if (workspace_bytes < detops_rle_decode_workspace_bytes(B, N)) return DETOPS_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const int64_t nchunks = chunks_of(B);
  const dim3 grid(static_cast<unsigned>(nchunks));
  int64_t* chunk_base = static_cast<int64_t*>(workspace);
  int64_t* chunk_sum = chunk_base + nchunks;
  int64_t* stat_chunk = chunk_sum + 2 * nchunks;
  int64_t* mask_sum = stat_chunk + kStats * nchunks;
  int64_t* stat_local = mask_sum + 2 * static_cast<int64_t>(N);
  hipLaunchKernelGGL(rle_decode_sums_kernel, grid, dim3(kBlock), 0, st, bytes, byte_offset, run_offset, N, B, chunk_base,
                     nchunks, chunk_sum, mask_sum);
  hipLaunchKernelGGL(rle_decode_sum_offsets_kernel, dim3(1), dim3(kBlock), 0, st, byte_offset, N, B, nchunks, chunk_sum,
                     mask_sum);
  hipLaunchKernelGGL(rle_decode_write_kernel, grid, dim3(kBlock), 0, st, bytes, byte_offset, run_offset, N, B, total,
                     chunk_base, nchunks, chunk_sum, mask_sum, counts, stat_chunk, stat_local);
  hipLaunchKernelGGL(rle_decode_status_kernel, dim3(1), dim3(kBlock), 0, st, bytes, byte_offset, N, B, nchunks, hw, stat_chunk,
                     stat_local, status);
  return launch_status();
}
