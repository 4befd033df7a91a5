// rle_string.hip — uncompressed COCO RLE (the run lengths of masker.hip's paste-RLE pair, or of any other encoder) to
// COCO's compressed strings, for gfx950 (MI355X).  The coding is defined in include/detops.h, "Compressed RLE strings".
//
//   detops_rle_string_count   bytes of every chunk of the flat run array, one scan over the chunks, the byte offset of
//                             every mask; [one host read of the total: byte_offset[N]]
//   detops_rle_string_write   the bytes: a chunk's strings are put together in LDS and leave in 16-byte stores
//
// The work is cut by chunks of kChunk runs of the FLAT array, never by mask: one detection has 50,000 runs and its
// neighbour three.  A thread owns kPer consecutive runs; a run finds its mask (the `i > 2` rule counts inside a mask) by
// a binary search in run_offset for the thread's first run and a walk from there.  A value's length is a closed form of
// its bit length, so both passes compute the same lengths and the offsets are plain prefix sums in a fixed order: no
// atomics, every output byte written exactly once, two runs give identical bytes.
#include "detops_dtype.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPer = 4;                          // consecutive runs of a thread
constexpr int kChunk = kBlock * kPer;            // runs of a workgroup
constexpr int kMaxLen = 7;                       // bytes of the difference of two int32 values at most
constexpr int kWaves = kBlock / kWave;
constexpr int kStageBytes = kChunk * kMaxLen + 32;   // a chunk's bytes behind a shift of up to 15, rounded up to 16

struct alignas(16) Line {                        // 16 bytes that move as one load and one store
  uint32_t w[4];
};

// bytes of the value x: the smallest k >= 1 with -2^(5k-1) <= x < 2^(5k-1)
__device__ __forceinline__ int code_len(int64_t x) {
  const unsigned long long y = static_cast<unsigned long long>(x < 0 ? ~x : x);
  const int bits = y ? 64 - __builtin_clzll(y) : 0;
  return (bits + 5) / 5;
}

struct ThreadRuns {
  int64_t x[kPer];      // the values to code: the run, minus the run two before it from the mask's fourth run on
  int len[kPer];        // their bytes (0: behind the end of the array)
  int mask[kPer];
  bool first[kPer];     // run 0 of its mask
  int sum;
};

__device__ __forceinline__ ThreadRuns load_runs(const int32_t* __restrict__ c, const int64_t* __restrict__ ro, int N,
                                                int64_t total, int64_t i0) {
  ThreadRuns r;
  r.sum = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    r.x[j] = 0;
    r.len[j] = 0;
    r.mask[j] = 0;
    r.first[j] = false;
  }
  if (i0 >= total) return r;
  int m = last_at_or_below(ro, N, i0);   // masks without runs share their successor's offset: the last one owns i0
  int64_t start = ro[m];
  int64_t next = m + 1 < N ? ro[m + 1] : INT64_MAX;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = i0 + j;
    if (i >= total) break;
    while (i >= next) {               // at most N steps, whatever run_offset holds
      ++m;
      start = next;
      next = m + 1 < N ? ro[m + 1] : INT64_MAX;
    }
    const int64_t k = i - start;
    int64_t v = c[i];
    if (k > 2 && i >= 2) v -= c[i - 2];
    r.x[j] = v;
    r.len[j] = code_len(v);
    r.mask[j] = m;
    r.first[j] = k == 0;
    r.sum += r.len[j];
  }
  return r;
}

// chunk_bytes[chunk] = bytes of the chunk; byte_offset[m] = bytes of the chunk in front of mask m's first run, written by
// the thread that owns that run (for every mask that has its first run, or would have it, at that position)
__global__ void __launch_bounds__(kBlock)
rle_string_count_kernel(const int32_t* __restrict__ c, const int64_t* __restrict__ ro, int N, int64_t total,
                        int64_t* __restrict__ chunk_bytes, int64_t* __restrict__ byte_offset) {
  __shared__ int wave_tot[kWaves];
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kPer;
  const ThreadRuns r = load_runs(c, ro, N, total, i0);
  int all;
  int off = block_scan<kBlock>(r.sum, wave_tot, all) - r.sum;
  if (threadIdx.x == 0) chunk_bytes[blockIdx.x] = all;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (r.first[j])
      for (int q = r.mask[j]; q >= 0 && ro[q] == i0 + j; --q) byte_offset[q] = off;
    off += r.len[j];
  }
}

// One workgroup: chunk_bytes to its exclusive sum in place (thread order within a tile of kBlock chunks, tiles in order),
// then byte_offset[m] = the base of the chunk of mask m's first run + what the count kernel left there; a mask that
// starts at the end of the array (entry N among them) gets the total
__global__ void __launch_bounds__(kBlock)
rle_string_offsets_kernel(const int64_t* __restrict__ ro, int N, int64_t total, int64_t nchunks,
                          int64_t* __restrict__ chunk_bytes, int64_t* __restrict__ byte_offset) {
  __shared__ int64_t wave_tot[kWaves];
  const int64_t carry = scan_tiles<kBlock>(
      nchunks, [&](int64_t b) { return chunk_bytes[b]; }, [&](int64_t b, int64_t before) { chunk_bytes[b] = before; }, wave_tot);
  for (int64_t j = threadIdx.x; j <= N; j += kBlock) {
    const int64_t first = ro[j];
    byte_offset[j] = (j == N || first >= total || first < 0) ? carry : chunk_bytes[first / kChunk] + byte_offset[j];
  }
}

// The chunk's bytes go to LDS at the offset they have modulo 16 in the output, so that every 16-byte line of LDS is one
// aligned 16-byte line of the output: full lines leave as one store per lane, the chunk's partial first and last line as
// the widest aligned pieces that fit (at most 4 stores each).
__global__ void __launch_bounds__(kBlock)
rle_string_write_kernel(const int32_t* __restrict__ c, const int64_t* __restrict__ ro, int N, int64_t total,
                        const int64_t* __restrict__ chunk_base, unsigned char* __restrict__ out) {
  __shared__ Line stage4[kStageBytes / 16];
  __shared__ int wave_tot[kWaves];
  unsigned char* stage = reinterpret_cast<unsigned char*>(stage4);
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(threadIdx.x) * kPer;
  const ThreadRuns r = load_runs(c, ro, N, total, i0);
  int all;
  const int off = block_scan<kBlock>(r.sum, wave_tot, all) - r.sum;
  unsigned char* dst = out + chunk_base[blockIdx.x];
  const int shift = static_cast<int>(reinterpret_cast<uintptr_t>(dst) & 15);
  int p = shift + off;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t x = r.x[j];
    for (int b = 0; b < r.len[j]; ++b) {
      const int ch = static_cast<int>((x >> (5 * b)) & 0x1f) | (b + 1 < r.len[j] ? 0x20 : 0);
      stage[p++] = static_cast<unsigned char>(ch + 48);
    }
  }
  __syncthreads();
  const int end = shift + all;
  unsigned char* line0 = dst - shift;               // 16-byte aligned; only [dst, dst + all) is touched
  for (int s = threadIdx.x; s * 16 < end; s += kBlock) {
    const int lo = max(s * 16, shift), hi = min(s * 16 + 16, end);
    if (hi - lo == 16) {
      *reinterpret_cast<Line*>(line0 + s * 16) = stage4[s];
      continue;
    }
    for (int b = lo; b < hi;) {
      if ((b & 7) == 0 && hi - b >= 8) {
        *reinterpret_cast<uint64_t*>(line0 + b) = *reinterpret_cast<const uint64_t*>(stage + b);
        b += 8;
      } else if ((b & 3) == 0 && hi - b >= 4) {
        *reinterpret_cast<uint32_t*>(line0 + b) = *reinterpret_cast<const uint32_t*>(stage + b);
        b += 4;
      } else if ((b & 1) == 0 && hi - b >= 2) {
        *reinterpret_cast<uint16_t*>(line0 + b) = *reinterpret_cast<const uint16_t*>(stage + b);
        b += 2;
      } else {
        line0[b] = stage[b];
        b += 1;
      }
    }
  }
}

int64_t chunks_of(int64_t total) { return (total + kChunk - 1) / kChunk; }

// 0: launch; 1: nothing to do; < 0: the error
int check_args(int64_t total, int N) {
  if (N < 0 || total < 0) return DETOPS_EINVAL;
  if (N == 0 || total == 0) return 1;
  if (chunks_of(total) > INT32_MAX) return DETOPS_EINVAL;
  return 0;
}

}  // namespace

DETOPS_API size_t detops_rle_string_workspace_bytes(int64_t total) {
  if (total <= 0) return 0;
  return static_cast<size_t>(chunks_of(total)) * sizeof(int64_t);
}

DETOPS_API int detops_rle_string_count(const int32_t* counts, const int64_t* run_offset, int64_t total, int N,
                                       int64_t* byte_offset, void* workspace, size_t workspace_bytes,
                                       detops_stream_t stream) {
  const int rc = check_args(total, N);
  if (rc) return rc < 0 ? rc : 0;
  if (!counts || !run_offset || !byte_offset || !workspace) return DETOPS_EINVAL;
  if (workspace_bytes < detops_rle_string_workspace_bytes(total)) return DETOPS_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const int64_t nchunks = chunks_of(total);
  int64_t* chunk_bytes = static_cast<int64_t*>(workspace);
  hipLaunchKernelGGL(rle_string_count_kernel, dim3(static_cast<unsigned>(nchunks)), dim3(kBlock), 0, st, counts, run_offset, N,
                     total, chunk_bytes, byte_offset);
  hipLaunchKernelGGL(rle_string_offsets_kernel, dim3(1), dim3(kBlock), 0, st, run_offset, N, total, nchunks, chunk_bytes,
                     byte_offset);
  return launch_status();
}

DETOPS_API int detops_rle_string_write(const int32_t* counts, const int64_t* run_offset, int64_t total, int N,
                                       const int64_t* byte_offset, uint8_t* out, const void* workspace,
                                       size_t workspace_bytes, detops_stream_t stream) {
  const int rc = check_args(total, N);
  if (rc) return rc < 0 ? rc : 0;
  if (!counts || !run_offset || !byte_offset || !out || !workspace) return DETOPS_EINVAL;
  if (workspace_bytes < detops_rle_string_workspace_bytes(total)) return DETOPS_EWORKSPACE;
  hipLaunchKernelGGL(rle_string_write_kernel, dim3(static_cast<unsigned>(chunks_of(total))), dim3(kBlock), 0,
                     as_stream(stream), counts, run_offset, N, total, static_cast<const int64_t*>(workspace), out);
  return launch_status();
}
