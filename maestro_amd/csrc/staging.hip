// Input staging: the median-date selection of multi-temporal rasters (maestro/dataset/dataset.py:188-220), one launch per modality
// per batch.  C ABI and the exact rule: include/maestro_hip.h.
//
// One workgroup per (sample, output date).  The rasters are tiny (C * S * S = 360 ... 2560 elements, windows of at most 64 dates):
// what costs is latency and launch count, not bandwidth.  A workgroup walks the raster in chunks of SD_CHUNK elements, one element
// per thread; the thread keeps its element's window as a column of LDS cells [W][SD_STRIDE] (consecutive lanes = consecutive
// elements: coalesced loads across the dates, conflict-free LDS columns), finds the two middle values by rank counting over
// that column, and overwrites the column with the deviations.  The per-date sums over a chunk then read the ROWS: integers are
// exact and are reduced wave-parallel in a fixed order; fp32 deviations are added in fp64 in element order by one lane per date
// (SD_STRIDE is odd, so the lanes of that loop sit on different banks).  No atomics, no per-thread array.
#include <type_traits>

#include "common.hpp"
#include "../../include/maestro_hip.h"

namespace {

constexpr int SD_THREADS = 256;
constexpr int SD_CHUNK = 240;                   // elements of one chunk, one per thread (the last 16 threads only help in the
                                                // strided phases): 64 dates * SD_STRIDE cells stay below the 64 KiB a launch may ask for
constexpr int SD_STRIDE = SD_CHUNK + 1;         // cells between two dates of the staged window
constexpr int SD_MAXW = MH_SELECT_MAX_WINDOW;

struct SdArgs {
    const void* raw;
    const unsigned char* mask;
    const short* dates;
    const int* t_start;
    const int* t_win;
    const double* scores;
    float* out;
    short* out_dates;
    int* out_index;
    long n_elem;
    int Cm, mask_floor, w_max, Tmax, nd, n_pix, log_scale;
    float norm_fac;
};

__device__ __forceinline__ bool sd_pixel_masked(const unsigned char* m, long date, int Cm, int n_pix, int p, int floor_) {
    const unsigned char* q = m + (size_t)date * Cm * n_pix + p;
    bool hit = false;
    for (int c = 0; c < Cm; ++c) hit = hit || (int)q[(size_t)c * n_pix] > floor_;
    return hit;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// T: the raw element type.  GIVEN: per-date scores come from the caller (random_dates), median and deviations are skipped.
template <typename T, bool GIVEN>
__global__ __launch_bounds__(SD_THREADS) void select_dates_kernel(const SdArgs A) {
    constexpr bool F32 = std::is_same<T, float>::value;
    using V = typename std::conditional<F32, float, int32_t>::type;      // what an LDS cell holds while it is a raw value
    extern __shared__ uint32_t cells[];                                  // [w_max][SD_STRIDE]; GIVEN: unused
    __shared__ unsigned long long score[SD_MAXW];                        // int64 sums, or the bits of the fp64 sums
    __shared__ unsigned char dirty[SD_MAXW];
    __shared__ int chosen;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x / A.nd, j = blockIdx.x - b * A.nd;
    const int W = A.t_win[b], ts = A.t_start[b];
    if (W < 1 || W > A.w_max || ts < 0 || (long)ts + (long)A.nd * W > (long)A.Tmax) {      // (uniform) the caller broke its promise
        if (tid == 0) A.out_index[blockIdx.x] = -1;
        return;
    }
    const long date0 = (long)b * A.Tmax + ts + (long)j * W;              // first raw date of the window, counted over the batch
    const T* raw = reinterpret_cast<const T*>(A.raw) + (size_t)date0 * A.n_elem;

    // ---- mask pre-pass: dirty dates, and the all-dirty fallback (dataset.py:196-199)
    if (tid < SD_MAXW) {
        dirty[tid] = 0;
        score[tid] = 0ull;                                               // int64 0 and fp64 +0.0
    }
    __syncthreads();
    if (A.mask) {
        const int n = W * A.n_pix;
        for (int i = tid; i < n; i += SD_THREADS) {
            const int w = i / A.n_pix, p = i - w * A.n_pix;
            if (sd_pixel_masked(A.mask, date0 + w, A.Cm, A.n_pix, p, A.mask_floor)) dirty[w] = 1;      // (every writer stores 1)
        }
        __syncthreads();
    }
    bool use_mask = false;
    if (A.mask) {
        bool all_dirty = true;
        for (int w = 0; w < W; ++w) all_dirty = all_dirty && dirty[w] != 0;
        use_mask = !all_dirty;
    }

    if (!GIVEN) {
        for (long e0 = 0; e0 < A.n_elem; e0 += SD_CHUNK) {
            const int cnt = (int)min((long)SD_CHUNK, A.n_elem - e0);
            uint32_t* col = cells + tid;
            if (tid < cnt) {
                const long e = e0 + tid;
                const int p = (int)(e % A.n_pix);
                unsigned long long valid = 0ull;                         // bit w: date w is unmasked at this element's pixel
                for (int w = 0; w < W; ++w) {
                    const V x = (V)raw[(size_t)w * A.n_elem + e];
                    col[w * SD_STRIDE] = __builtin_bit_cast(uint32_t, x);
                    if (!use_mask || !sd_pixel_masked(A.mask, date0 + w, A.Cm, A.n_pix, p, A.mask_floor)) valid |= 1ull << w;
                }
                // the two middle values of the valid ones by rank counting: x is the k-th smallest (0-based) iff
                // #{< x} <= k < #{<= x}.  At least one date is valid (a clean date exists whenever the mask is in use).
                const int n = __popcll(valid), k1 = (n - 1) >> 1, k2 = n >> 1;
                V lo = 0, hi = 0;
                for (int i = 0; i < W; ++i) {
                    if (!((valid >> i) & 1ull)) continue;
                    const V xi = __builtin_bit_cast(V, col[i * SD_STRIDE]);
                    int lt = 0, le = 0;
                    for (int k = 0; k < W; ++k) {
                        const V xk = __builtin_bit_cast(V, col[k * SD_STRIDE]);
                        const bool ok = (valid >> k) & 1ull;
                        lt += (ok && xk < xi) ? 1 : 0;
                        le += (ok && xk <= xi) ? 1 : 0;
                    }
                    if (lt <= k1 && k1 < le) lo = xi;
                    if (lt <= k2 && k2 < le) hi = xi;
                }
                // the column becomes the deviations (masked elements belong to dirty dates, which are out: 0)
                if constexpr (F32) {
                    const float med = k1 == k2 ? lo : (lo + hi) / 2.0f;           // numpy: mean of the one or two middle values in fp32
                    for (int w = 0; w < W; ++w) {
                        const float x = __builtin_bit_cast(float, col[w * SD_STRIDE]);
                        col[w * SD_STRIDE] = ((valid >> w) & 1ull) ? __builtin_bit_cast(uint32_t, fabsf(x - med)) : 0u;
                    }
                } else {
                    const int32_t s2 = lo + hi;                                    // |2x - (a + b)| <= 2^18: exact in 32 bits
                    for (int w = 0; w < W; ++w) {
                        const int32_t d = 2 * __builtin_bit_cast(int32_t, col[w * SD_STRIDE]) - s2;
                        col[w * SD_STRIDE] = ((valid >> w) & 1ull) ? (uint32_t)(d < 0 ? -d : d) : 0u;
                    }
                }
            }
            __syncthreads();
            // ---- per-date sums of the chunk, fixed order
            if constexpr (F32) {
                if (tid < W) {                                                     // one lane per date: fp64, element order
                    const uint32_t* row = cells + tid * SD_STRIDE;
                    double acc = __builtin_bit_cast(double, score[tid]);
#pragma unroll 8
                    for (int i = 0; i < cnt; ++i) acc += (double)__builtin_bit_cast(float, row[i]);
                    score[tid] = __builtin_bit_cast(unsigned long long, acc);
                }
            } else {
                for (int w = wv; w < W; w += SD_THREADS / 64) {                    // one wave per date: integers, any order is exact
                    const uint32_t* row = cells + w * SD_STRIDE;
                    long long s = 0;
                    for (int i = lane; i < cnt; i += 64) s += (long long)row[i];
                    s = wave_sum_i64(s);
                    if (lane == 0) score[w] += (unsigned long long)s;
                }
            }
            __syncthreads();
        }
    }

    // ---- one lane picks the date (nanargmin: the lowest score among the clean dates, the lowest index among equals)
    if (tid == 0) {
        int best = -1;
        if (GIVEN) {
            double bs = 0.0;
            for (int w = 0; w < W; ++w) {
                if (use_mask && dirty[w]) continue;
                const double s = A.scores[date0 + w];
                if (s != s) continue;
                if (best < 0 || s < bs) { best = w; bs = s; }
            }
        } else if (F32) {
            double bs = 0.0;
            for (int w = 0; w < W; ++w) {
                if (use_mask && dirty[w]) continue;
                const double s = __builtin_bit_cast(double, score[w]);
                if (best < 0 || s < bs) { best = w; bs = s; }
            }
        } else {
            long long bs = 0;
            for (int w = 0; w < W; ++w) {
                if (use_mask && dirty[w]) continue;
                const long long s = (long long)score[w];
                if (best < 0 || s < bs) { best = w; bs = s; }
            }
        }
        if (best < 0) best = 0;
        chosen = best;
        A.out_index[blockIdx.x] = best;
        const short* d = A.dates + (size_t)(date0 + best) * 3;
        short* od = A.out_dates + (size_t)blockIdx.x * 3;
        od[0] = d[0]; od[1] = d[1]; od[2] = d[2];
    }
    __syncthreads();

    // ---- the whole workgroup writes the chosen date: float cast, log, one correctly rounded division (dataset.py:215-220)
    const T* src = raw + (size_t)chosen * A.n_elem;
    float* dst = A.out + (size_t)blockIdx.x * A.n_elem;
    const bool div = A.norm_fac > 0.f;
    for (long e = tid; e < A.n_elem; e += SD_THREADS) {
        float x = (float)src[e];
        if (A.log_scale) x = logf(x < 1e-10f ? 1e-10f : x);
        if (div) x = __fdiv_rn(x, A.norm_fac);
        dst[e] = x;
    }
}

template <typename T>
void sd_launch(const SdArgs& A, int B, bool given, hipStream_t s) {
    const dim3 grid((unsigned)((long)B * A.nd)), block(SD_THREADS);
    if (given)
        hipLaunchKernelGGL((select_dates_kernel<T, true>), grid, block, 0, s, A);
    else
        hipLaunchKernelGGL((select_dates_kernel<T, false>), grid, block, (size_t)A.w_max * SD_STRIDE * sizeof(uint32_t), s, A);
}

}  // namespace

extern "C" int mh_select_dates(const void* raw, int raw_code, const unsigned char* mask, int Cm, int mask_floor, const short* dates,
                               const int* t_start, const int* t_win, int w_max, const double* scores, float* out, short* out_dates,
                               int* out_index, int B, int Tmax, int nd, long n_elem, int n_pix, int log_scale, float norm_fac,
                               void* stream) {
    MH_CHECK_ARG(raw && dates && t_start && t_win && out && out_dates && out_index, "mh_select_dates: null pointer");
    MH_CHECK_ARG(raw_code >= MH_RAW_U8 && raw_code <= MH_RAW_F32, "mh_select_dates: element code %d (0 = u8, 1 = i16, 2 = u16, 3 = f32)",
                 raw_code);
    MH_CHECK_ARG(w_max >= 1 && w_max <= SD_MAXW, "mh_select_dates: window of %d dates (1 ... %d are supported)", w_max, SD_MAXW);
    MH_CHECK_ARG(B > 0 && nd > 0 && Tmax > 0, "mh_select_dates: B, nd, Tmax must be positive (got %d, %d, %d)", B, nd, Tmax);
    MH_CHECK_ARG((long)nd * w_max <= (long)Tmax, "mh_select_dates: %d windows of %d dates do not fit Tmax = %d", nd, w_max, Tmax);
    MH_CHECK_ARG((long)B * nd <= 0x7fffffffL, "mh_select_dates: B * nd = %ld too large", (long)B * nd);
    MH_CHECK_ARG(n_pix >= 1 && n_elem >= 1 && n_elem <= 0x7fffffffL && n_elem % n_pix == 0,
                 "mh_select_dates: n_elem = %ld must be a positive multiple of n_pix = %d", n_elem, n_pix);
    MH_CHECK_ARG(!mask || Cm >= 1, "mh_select_dates: a mask of %d channels", Cm);
    SdArgs A;
    A.raw = raw; A.mask = mask; A.dates = dates; A.t_start = t_start; A.t_win = t_win; A.scores = scores;
    A.out = out; A.out_dates = out_dates; A.out_index = out_index;
    A.n_elem = n_elem; A.Cm = Cm; A.mask_floor = mask_floor; A.w_max = w_max; A.Tmax = Tmax; A.nd = nd; A.n_pix = n_pix;
    A.log_scale = log_scale; A.norm_fac = norm_fac;
    hipStream_t s = (hipStream_t)stream;
    switch (raw_code) {
        case MH_RAW_U8: sd_launch<uint8_t>(A, B, scores != nullptr, s); break;
        case MH_RAW_I16: sd_launch<int16_t>(A, B, scores != nullptr, s); break;
        case MH_RAW_U16: sd_launch<uint16_t>(A, B, scores != nullptr, s); break;
        default: sd_launch<float>(A, B, scores != nullptr, s); break;
    }
    MH_LAUNCH_CHECK();
    return 0;
}
