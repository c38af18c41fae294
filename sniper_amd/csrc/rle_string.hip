// rle_string.hip -- compressed string counts on the device: rleToString and rleFrString (lib/dataset/pycocotools/maskApi.c:181-208),
// the `counts` of a COCO results file.  Integer arithmetic, exact bytes.
//
// A count is coded in k characters of six bits from chr(48): five of payload, 0x20 = another character follows, 0x10 of the last one =
// the sign; from the fourth count on the value coded is the difference to the count two before.  Masks and strings are pooled behind
// (N+1) int32 offsets.  One workgroup of ONE wave per mask: the masks of a results file have tens of counts, so a wider workgroup would
// idle, and a wave needs neither LDS nor a barrier.  The lanes take kChunk = 64 counts (characters) at a time and a carry goes from
// chunk to chunk, the same in every lane.
//   rle_string_len_kernel   k of every count, summed over the wave.
//   rle_to_string_kernel    an exclusive scan of k places every count's characters; each lane stores its k bytes.  Byte stores straight
//                           to HBM: a string starts at any byte, so dword stores from an LDS image would need a head and a tail path;
//                           neighbouring lanes write neighbouring bytes and the caches merge them.
//   rle_string_count_kernel per character: is it the last of its count, is it inside chr(48) .. chr(111), does it close seven
//                           continuation characters in a row; sums and ORs over the wave give m and the status.
//   rle_from_string_kernel  the lane of a count's LAST character walks back over its (at most six) continuation characters and forms
//                           x; the count's index is the scan of the last-character flags; cnts[i] = x_i + cnts[i-2] (i > 2) is two
//                           interleaved prefix sums modulo 2^32 -- over the odd i and over the even i >= 2 -- scanned with carries.
// No atomics, no scratch, no workspace; every output element is written once, in one fixed order.
#include "common.h"
#include "eval_order.h"

namespace {

constexpr int kThreads = kWave;        // one wave per mask
constexpr int kChunk = kThreads;       // counts / characters per step
constexpr int kMaxChars = 7;           // of one count: 5 * 7 = 35 bits hold any difference of two uint32

__device__ __forceinline__ unsigned wave_scan_add_u(unsigned v, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// the value coded for count i and the number of its characters
__device__ __forceinline__ int coded(const uint32_t *__restrict__ c, int i, long long &x) {
  x = (long long)c[i] - (i > 2 ? (long long)c[i - 2] : 0ll);
  int k = 1;
#pragma unroll
  for (; k < kMaxChars; ++k) {
    const long long lim = 1ll << (5 * k - 1);
    if (x >= -lim && x < lim) break;
  }
  return k;
}

__global__ __launch_bounds__(kThreads) void rle_string_len_kernel(const uint32_t *__restrict__ cnts, const int32_t *__restrict__ run_off,
                                                                  int32_t *__restrict__ str_len) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int o0 = run_off[n], m = run_off[n + 1] - o0;
  const uint32_t *c = cnts + o0;
  int total = 0;
  for (int base = 0; base < m; base += kChunk) {
    const int i = base + lane;
    long long x;
    total += i < m ? coded(c, i, x) : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
  if (lane == 0) str_len[n] = total;
}

__global__ __launch_bounds__(kThreads) void rle_to_string_kernel(const uint32_t *__restrict__ cnts, const int32_t *__restrict__ run_off,
                                                                 const int32_t *__restrict__ str_off, uint8_t *__restrict__ chars) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int o0 = run_off[n], m = run_off[n + 1] - o0;
  const int s0 = str_off[n], L = str_off[n + 1] - s0;
  const uint32_t *c = cnts + o0;
  uint8_t *out = chars + s0;
  int carry = 0;
  for (int base = 0; base < m; base += kChunk) {
    const int i = base + lane;
    long long x = 0;
    const int k = i < m ? coded(c, i, x) : 0;
    const int inc = wave_scan_add(k, lane);
    const int at = carry + inc - k;
    for (int j = 0; j < k; ++j) {
      const int ch = (int)((x >> (5 * j)) & 0x1f) | (j < k - 1 ? 0x20 : 0);
      if (at + j < L) out[at + j] = (uint8_t)(ch + 48);       // (L is what the length pass found: never past the mask's slots)
    }
    carry += __shfl(inc, kWave - 1, 64);
  }
}

__global__ __launch_bounds__(kThreads) void rle_string_count_kernel(const uint8_t *__restrict__ chars, const int32_t *__restrict__ str_off,
                                                                    int32_t *__restrict__ m_out, int32_t *__restrict__ status) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int s0 = str_off[n], L = str_off[n + 1] - s0;
  const uint8_t *s = chars + s0;
  int last = 0, bad = 0;                  // bad: 1 = a foreign character, 2 = a count of more than kMaxChars characters
  for (int base = 0; base < L; base += kChunk) {
    const int p = base + lane;
    if (p < L) {
      const int c = (int)s[p] - 48;
      if (c < 0 || c > 63) bad |= 1;
      if (!(c & 0x20)) ++last;
      if (p >= kMaxChars - 1) {           // characters p - 6 .. p all ask for another one: the count has at least eight
        bool run = true;
#pragma unroll
        for (int j = 0; j < kMaxChars; ++j) run = run && (((int)s[p - j] - 48) & 0x20);
        if (run) bad |= 2;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    last += __shfl_xor(last, off, 64);
    bad |= __shfl_xor(bad, off, 64);
  }
  if (lane == 0) {
    const bool open = L > 0 && ((((int)s[L - 1] - 48) & 0x20) != 0);
    m_out[n] = last;
    status[n] = (bad & 1) ? 2 : (open ? 1 : ((bad & 2) ? 3 : 0));
  }
}

__global__ __launch_bounds__(kThreads) void rle_from_string_kernel(const uint8_t *__restrict__ chars, const int32_t *__restrict__ str_off,
                                                                   const int32_t *__restrict__ run_off, const int32_t *__restrict__ status,
                                                                   uint32_t *__restrict__ cnts) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (status[n] != 0) return;             // (uniform over the workgroup)
  const int s0 = str_off[n], L = str_off[n + 1] - s0;
  const int o0 = run_off[n], m = run_off[n + 1] - o0;
  const uint8_t *s = chars + s0;
  uint32_t *out = cnts + o0;
  int idx_carry = 0;
  unsigned even_carry = 0, odd_carry = 0;
  for (int base = 0; base < L; base += kChunk) {
    const int p = base + lane;
    const int c = p < L ? (int)s[p] - 48 : 0x20;
    const bool last = !(c & 0x20);
    unsigned x = 0;
    if (last) {
      int k = 1;                          // the characters of this count: status 0 says at most kMaxChars
      while (k < kMaxChars && p - k >= 0 && (((int)s[p - k] - 48) & 0x20)) ++k;
      for (int j = 0; j < k; ++j) {
        const unsigned pay = (unsigned)(((int)s[p - (k - 1) + j] - 48) & 0x1f);
        if (5 * j < 32) x |= pay << (5 * j);
      }
      if ((c & 0x10) && 5 * k < 32) x |= ~0u << (5 * k);
    }
    const int inc = wave_scan_add(last ? 1 : 0, lane);
    const int i = idx_carry + inc - 1;    // this count's index, where `last`
    const bool odd = last && (i & 1), even = last && !(i & 1) && i >= 2;        // the two chains; count 0 belongs to neither
    const unsigned so = wave_scan_add_u(odd ? x : 0u, lane), se = wave_scan_add_u(even ? x : 0u, lane);
    if (last && i < m) out[i] = i == 0 ? x : (odd ? odd_carry + so : even_carry + se);
    idx_carry += __shfl(inc, kWave - 1, 64);
    odd_carry += __shfl(so, kWave - 1, 64);
    even_carry += __shfl(se, kWave - 1, 64);
  }
}

// h_off (HOST, N+1): starts at 0, never decreases, ends at `total`
const char *bad_offsets(const int32_t *h_off, long N, long total) {
  if (h_off[0] != 0) return "do not start at 0";
  for (long n = 0; n < N; ++n)
    if (h_off[n + 1] < h_off[n]) return "decrease";
  if ((long)h_off[N] != total) return "do not end at the total given";
  return nullptr;
}

}  // namespace

#define SN_RLE_STRING_COMMON(fn, N, total_runs, total_chars)                                                                          \
  SN_REQUIRE(N >= 1 && N < 2147483647L, fn ": 1 <= N < 2^31 - 1 required (N = %ld)", (long)(N));                                      \
  SN_REQUIRE(total_runs >= 0 && total_runs < 2147483648L,                                                                            \
             fn ": the counts of a call must fit 32-bit indexing, 0 <= total_runs < 2^31 required (total_runs = %ld)", (long)(total_runs)); \
  SN_REQUIRE(total_chars >= 0 && total_chars < 2147483648L,                                                                          \
             fn ": the characters of a call must fit 32-bit indexing, 0 <= total_chars < 2^31 required (total_chars = %ld)", (long)(total_chars))
#define SN_RLE_STRING_OFFSETS(fn, name, h_off, N, total)                            \
  do {                                                                              \
    const char *why__ = bad_offsets(h_off, N, total);                               \
    SN_REQUIRE(!why__, fn ": the offsets " name " %s (N = %ld, total = %ld)", why__, (long)(N), (long)(total)); \
  } while (0)

SN_EXPORT int sn_rle_string_limits(int32_t *h_out3) {
  SN_REQUIRE(h_out3, "sn_rle_string_limits: null pointer");
  h_out3[0] = kThreads;
  h_out3[1] = kChunk;
  h_out3[2] = kMaxChars;
  return SN_OK;
}

SN_EXPORT int sn_rle_string_len(const uint32_t *cnts, const int32_t *run_off, const int32_t *h_run_off, long N, long total_runs,
                                int32_t *str_len, sn_stream_t stream) {
  SN_REQUIRE(cnts && run_off && h_run_off && str_len, "sn_rle_string_len: null pointer");
  SN_RLE_STRING_COMMON("sn_rle_string_len", N, total_runs, 0L);
  SN_RLE_STRING_OFFSETS("sn_rle_string_len", "run_off", h_run_off, N, total_runs);
  hipLaunchKernelGGL(rle_string_len_kernel, dim3((unsigned)N), dim3(kThreads), 0, sn_stream(stream), cnts, run_off, str_len);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_rle_to_string(const uint32_t *cnts, const int32_t *run_off, const int32_t *h_run_off, const int32_t *str_off,
                               const int32_t *h_str_off, long N, long total_runs, long total_chars, uint8_t *chars, sn_stream_t stream) {
  SN_REQUIRE(cnts && run_off && h_run_off && str_off && h_str_off && chars, "sn_rle_to_string: null pointer");
  SN_RLE_STRING_COMMON("sn_rle_to_string", N, total_runs, total_chars);
  SN_RLE_STRING_OFFSETS("sn_rle_to_string", "run_off", h_run_off, N, total_runs);
  SN_RLE_STRING_OFFSETS("sn_rle_to_string", "str_off", h_str_off, N, total_chars);
  hipLaunchKernelGGL(rle_to_string_kernel, dim3((unsigned)N), dim3(kThreads), 0, sn_stream(stream), cnts, run_off, str_off, chars);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_rle_string_count(const uint8_t *chars, const int32_t *str_off, const int32_t *h_str_off, long N, long total_chars,
                                  int32_t *m, int32_t *status, sn_stream_t stream) {
  SN_REQUIRE(chars && str_off && h_str_off && m && status, "sn_rle_string_count: null pointer");
  SN_RLE_STRING_COMMON("sn_rle_string_count", N, 0L, total_chars);
  SN_RLE_STRING_OFFSETS("sn_rle_string_count", "str_off", h_str_off, N, total_chars);
  hipLaunchKernelGGL(rle_string_count_kernel, dim3((unsigned)N), dim3(kThreads), 0, sn_stream(stream), chars, str_off, m, status);
  SN_CHECK_LAUNCH();
  return SN_OK;
}

SN_EXPORT int sn_rle_from_string(const uint8_t *chars, const int32_t *str_off, const int32_t *h_str_off, const int32_t *run_off,
                                 const int32_t *h_run_off, const int32_t *status, long N, long total_chars, long total_runs,
                                 uint32_t *cnts, sn_stream_t stream) {
  SN_REQUIRE(chars && str_off && h_str_off && run_off && h_run_off && status && cnts, "sn_rle_from_string: null pointer");
  SN_RLE_STRING_COMMON("sn_rle_from_string", N, total_runs, total_chars);
  SN_RLE_STRING_OFFSETS("sn_rle_from_string", "str_off", h_str_off, N, total_chars);
  SN_RLE_STRING_OFFSETS("sn_rle_from_string", "run_off", h_run_off, N, total_runs);
  hipLaunchKernelGGL(rle_from_string_kernel, dim3((unsigned)N), dim3(kThreads), 0, sn_stream(stream), chars, str_off, run_off, status, cnts);
  SN_CHECK_LAUNCH();
  return SN_OK;
}
