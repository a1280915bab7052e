// Keyframe selection and window management on the device: the three quantities the tracker decides from
// (/root/reference/utils/slam_tracker.py:192-284, 412-452) and the decision itself, without a host synchronisation.
//
//   mgs_masked_median   median of the tracked render's depth (get_median_depth, /root/reference/utils/slam_utils.py:149-157):
//                       an exact radix select on an order-preserving 32-bit key, three digit passes (11 + 11 + 10 bits).
//                       Every pass is two launches: a histogram launch in which each workgroup counts its share of the
//                       elements in LDS and stores its OWN row of partial counts, and a one-workgroup launch that adds the
//                       rows in a fixed order, finds the bucket that holds the wanted rank and narrows the key prefix.  Six
//                       launches whatever the data; nothing waits on another workgroup inside a launch, nothing is cleared,
//                       every word that is read was written earlier in the same call.
//   mgs_covisibility    |A and B_k|, |A or B_k|, |A|, |B_k| of the current frame's n_touched > 0 set against the packed
//                       visibility rows of the window (the words mgs_window_stats leaves): popcounts, one integer atomic add
//                       per workgroup, keyframe and field behind a memset node -- integer sums do not depend on their order.
//   mgs_keyframe_decide one wave: the keyframe test and both evictions of add_to_window from those counts, the median and the
//                       poses; eight words for the host to read once per tracked frame.
//
// Counting is integer throughout, so the results are bitwise reproducible; the comparisons that select elements are made on
// the integer keys, so they do not depend on the denormal mode either.
#include <math.h>

#include "common.h"

namespace mgs {

// ---- masked median ---------------------------------------------------------------------------------------------------
constexpr int MD_THREADS = 256;
constexpr int MD_BINS = 2048;               // 11-bit digits (the last pass uses 10 bits: 1024 bins)
constexpr int MD_MAX_WG = 64;               // rows of partial counts the select launch adds
constexpr int MD_PER_WG = 4096;             // elements a workgroup counts before another one is worth its row
enum : int { MD_PREFIX = 0, MD_RANK = 1, MD_COUNT = 2, MD_HDR = 16 };    // scratch: 16 header words, then [G][MD_BINS] counts

__host__ __device__ inline int md_pass_bits(int pass) { return pass == 2 ? 10 : 11; }
__host__ __device__ inline int md_pass_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }

static unsigned md_workgroups(uint64_t n) {
    const uint64_t g = (n + MD_PER_WG - 1) / MD_PER_WG;
    return (unsigned)(g < 1 ? 1 : g > MD_MAX_WG ? MD_MAX_WG : g);
}

// float bits -> a key whose unsigned order is the order of the floats (-0 and +0 share the key of +0)
__host__ __device__ inline uint32_t md_key(uint32_t u) {
    if ((u << 1) == 0) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline uint32_t md_unkey(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

template <int PASS>
__global__ void __launch_bounds__(MD_THREADS) median_hist_kernel(const uint32_t* __restrict__ values,
                                                                 const uint32_t* __restrict__ mask, uint64_t n, uint32_t lo_key,
                                                                 uint32_t* __restrict__ scratch) {
    __shared__ uint32_t s_hist[MD_BINS];
    constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
    constexpr int NB = PASS == 2 ? 1024 : 2048;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int b = tid; b < NB; b += MD_THREADS) s_hist[b] = 0;
    const uint32_t prefix = PASS == 0 ? 0u : scratch[MD_PREFIX];      // written by the previous pass's select launch
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * MD_THREADS;
    for (uint64_t base = (uint64_t)blockIdx.x * MD_THREADS; base < n; base += stride) {    // uniform trip count per wave
        const uint64_t i = base + tid;
        bool pend = false;
        uint32_t digit = 0;
        if (i < n) {
            const uint32_t key = md_key(values[i]);
            pend = key > lo_key && (!mask || (mask[i] << 1) != 0);
            if (PASS > 0) pend = pend && ((key ^ prefix) >> (SHIFT + (PASS == 1 ? 11 : 10))) == 0;
            digit = (key >> SHIFT) & (NB - 1);
        }
        // a depth image falls into a handful of buckets: the lanes that share the first pending lane's digit add once
        const unsigned long long act = __builtin_amdgcn_ballot_w64(pend);
        if (act) {
            const int leader = __ffsll((long long)act) - 1;
            const uint32_t d0 = (uint32_t)__shfl((int)digit, leader);
            const unsigned long long same = __builtin_amdgcn_ballot_w64(pend && digit == d0);
            if (lane == leader) atomicAdd(&s_hist[d0], (uint32_t)__popcll(same));
            pend = pend && digit != d0;
        }
        if (pend) atomicAdd(&s_hist[digit], 1u);
    }
    __syncthreads();
    uint32_t* row = scratch + MD_HDR + (size_t)blockIdx.x * MD_BINS;
    for (int b = tid; b < NB; b += MD_THREADS) row[b] = s_hist[b];
}

// adds the G rows bucket by bucket (row 0 first), then walks the buckets in ascending order to the one that holds the rank
template <int PASS>
__global__ void __launch_bounds__(MD_THREADS) median_select_kernel(uint32_t* __restrict__ scratch, int G,
                                                                   float* __restrict__ out_median,
                                                                   uint32_t* __restrict__ out_count) {
    __shared__ uint32_t s_tot[MD_BINS];
    __shared__ uint32_t s_scan[MD_THREADS];
    constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
    constexpr int NB = PASS == 2 ? 1024 : 2048;
    constexpr int CH = NB / MD_THREADS;                                // consecutive buckets per thread
    const int tid = threadIdx.x;
    for (int b = tid; b < NB; b += MD_THREADS) {
        uint32_t t = 0;
        for (int g = 0; g < G; ++g) t += scratch[MD_HDR + (size_t)g * MD_BINS + b];
        s_tot[b] = t;
    }
    __syncthreads();
    uint32_t chunk = 0;
    for (int j = 0; j < CH; ++j) chunk += s_tot[tid * CH + j];
    s_scan[tid] = chunk;
    __syncthreads();
    for (int off = 1; off < MD_THREADS; off <<= 1) {                   // inclusive scan of the 256 chunk sums
        const uint32_t add = tid >= off ? s_scan[tid - off] : 0u;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const uint32_t total = s_scan[MD_THREADS - 1];
    uint32_t count, rank, prefix;
    if (PASS == 0) { count = total; rank = count ? (count - 1) / 2 : 0; prefix = 0; }
    else { count = scratch[MD_COUNT]; rank = scratch[MD_RANK]; prefix = scratch[MD_PREFIX]; }
    __syncthreads();                                                   // every thread holds the header before one rewrites it
    uint32_t excl = s_scan[tid] - chunk;
    if (count != 0 && rank >= excl && rank - excl < chunk) {           // exactly one thread
        int b = tid * CH;
        while (rank - excl >= s_tot[b]) { excl += s_tot[b]; ++b; }
        prefix |= (uint32_t)b << SHIFT;
        if (PASS < 2) {
            scratch[MD_PREFIX] = prefix; scratch[MD_RANK] = rank - excl; scratch[MD_COUNT] = count;
        } else {
            *out_median = __uint_as_float(md_unkey(prefix));
            *out_count = count;
        }
    }
    if (count == 0 && tid == 0) {
        if (PASS < 2) {
            scratch[MD_PREFIX] = 0; scratch[MD_RANK] = 0; scratch[MD_COUNT] = 0;
        } else {
            *out_median = __uint_as_float(0x7fc00000u);
            *out_count = 0;
        }
    }
}

template <int PASS>
static void median_pass(const uint32_t* values, const uint32_t* mask, uint64_t n, uint32_t lo_key, uint32_t* scratch, int G,
                        float* out_median, uint32_t* out_count, hipStream_t s) {
    hipLaunchKernelGGL(median_hist_kernel<PASS>, dim3(G), dim3(MD_THREADS), 0, s, values, mask, n, lo_key, scratch);
    hipLaunchKernelGGL(median_select_kernel<PASS>, dim3(1), dim3(MD_THREADS), 0, s, scratch, G, out_median, out_count);
}

// ---- covisibility counts ---------------------------------------------------------------------------------------------
constexpr int KW_MAX_KF = 32;
constexpr int CV_THREADS = 256;
constexpr int CV_WAVES = CV_THREADS / 64;
constexpr int CV_MAX_WG = 128;
struct CovisArgs {
    const unsigned long long* kf_bits[KW_MAX_KF];
    uint32_t kf_words[KW_MAX_KF];           // clamped to `words`: a shorter row reads as zero beyond its end
    const int32_t* cur_n_touched;
    const unsigned long long* cur_bits;
    unsigned long long* cur_out;
    uint32_t* counts;                       // [K][4], zeroed by the memset node in front
    int K, P;
    uint32_t words;
};
__global__ void __launch_bounds__(CV_THREADS) covisibility_kernel(CovisArgs a) {
    __shared__ uint32_t s_part[CV_WAVES][KW_MAX_KF][3];
    __shared__ uint32_t s_a[CV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool row = lane < a.K;
    const unsigned long long* bits = nullptr;
    uint32_t row_words = 0;
    if (row) { bits = a.kf_bits[lane]; row_words = a.kf_words[lane]; }
    uint32_t c_and = 0, c_or = 0, c_b = 0, c_a = 0;
    const uint32_t step = gridDim.x * CV_WAVES;
    for (uint32_t w = blockIdx.x * CV_WAVES + wave; w < a.words; w += step) {      // one word per wave and trip
        const unsigned long long tail = (w == a.words - 1 && (a.P & 63)) ? ((1ull << (a.P & 63)) - 1ull) : ~0ull;
        unsigned long long A;
        if (a.cur_n_touched) {
            const size_t i = (size_t)w * 64 + lane;
            A = __builtin_amdgcn_ballot_w64(i < (size_t)a.P && a.cur_n_touched[i] > 0);
        } else {
            A = a.cur_bits[w] & tail;
        }
        if (a.cur_out && lane == 0) a.cur_out[w] = A;
        c_a += (uint32_t)__popcll(A);
        if (row) {
            const unsigned long long B = (w < row_words ? bits[w] : 0ull) & tail;
            c_and += (uint32_t)__popcll(A & B);
            c_or += (uint32_t)__popcll(A | B);
            c_b += (uint32_t)__popcll(B);
        }
    }
    if (lane < KW_MAX_KF) { s_part[wave][lane][0] = c_and; s_part[wave][lane][1] = c_or; s_part[wave][lane][2] = c_b; }
    if (lane == 0) s_a[wave] = c_a;
    __syncthreads();
    if (tid < a.K) {
        uint32_t t_and = 0, t_or = 0, t_b = 0, t_a = 0;
        for (int v = 0; v < CV_WAVES; ++v) {
            t_and += s_part[v][tid][0]; t_or += s_part[v][tid][1]; t_b += s_part[v][tid][2]; t_a += s_a[v];
        }
        uint32_t* c = a.counts + 4 * tid;
        atomicAdd(c + 0, t_and); atomicAdd(c + 1, t_or); atomicAdd(c + 2, t_a); atomicAdd(c + 3, t_b);
    }
}

// ---- the decision ----------------------------------------------------------------------------------------------------
constexpr int KD_MAX = KW_MAX_KF + 1;       // list positions: the current frame, then the window, most recent first
struct DecideArgs {
    MgsKeyframeParams p;
    const uint32_t* counts;
    const float* median;
    const float* R[KD_MAX];
    const float* T[KD_MAX];
    uint32_t* out;
};
// || t(T_i T_j^-1) || for world->camera poses: T_i T_j^-1 = [R_i R_j^T, t_i - R_i R_j^T t_j]
__device__ inline float kd_distance(const float* Ri, const float* ti, const float* Rj, const float* tj) {
    float u[3], v[3];
    for (int c = 0; c < 3; ++c) u[c] = Rj[0 + c] * tj[0] + Rj[3 + c] * tj[1] + Rj[6 + c] * tj[2];
    for (int r = 0; r < 3; ++r) v[r] = ti[r] - (Ri[3 * r] * u[0] + Ri[3 * r + 1] * u[1] + Ri[3 * r + 2] * u[2]);
    return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}
__global__ void __launch_bounds__(64) keyframe_decide_kernel(DecideArgs a) {
    __shared__ float s_R[KD_MAX][9];
    __shared__ float s_T[KD_MAX][3];
    __shared__ float s_score[KD_MAX];
    const int lane = threadIdx.x;
    const MgsKeyframeParams& p = a.p;
    const int K = p.K, n = K + 1, ndt = p.n_dont_touch;
    float R[9], T[3];
    for (int e = 0; e < 9; ++e) R[e] = 0.f;
    for (int e = 0; e < 3; ++e) T[e] = 0.f;
    if (lane < n) {
        const float* gr = a.R[lane];
        const float* gt = a.T[lane];
        for (int e = 0; e < 9; ++e) s_R[lane][e] = R[e] = gr[e];
        for (int e = 0; e < 3; ++e) s_T[lane][e] = T[e] = gt[e];
    }
    __syncthreads();
    const float median = a.median[0];
    const uint32_t n_a = a.counts[2];
    // positions ndt..K of the new list [cur] + window: Szymkiewicz-Simpson overlap with the current frame
    const bool movable = lane >= ndt && lane <= K;
    bool cand = false;
    if (movable) {
        const uint32_t* c = a.counts + 4 * (lane - 1);
        const uint32_t n_b = c[3];
        const float r = (float)c[0] / (float)(n_a < n_b ? n_a : n_b);
        cand = r <= (p.window_full ? p.kf_cutoff : 0.4f);              // NaN compares false
    }
    const unsigned long long cands = __builtin_amdgcn_ballot_w64(cand);
    const int cut = cands ? 63 - __clzll((long long)cands) : -1;        // only the last candidate goes
    const int len = n - (cut >= 0 ? 1 : 0);
    int by_size = -1;
    if (len > p.window_size) {                                          // wave-uniform
        const bool alive = movable && lane != cut;
        float score = 0.f;
        if (alive) {
            float sum = 0.f;
            for (int j = ndt; j <= K; ++j) {
                if (j == lane || j == cut) continue;
                sum += 1.0f / (kd_distance(R, T, s_R[j], s_T[j]) + 1e-6f);
            }
            score = sqrtf(kd_distance(R, T, s_R[0], s_T[0])) * sum;
        }
        if (lane < KD_MAX) s_score[lane] = score;
        __syncthreads();
        if (lane == 0) {
            float best = -INFINITY;
            for (int i = ndt; i <= K; ++i)
                if (i != cut && s_score[i] > best) { best = s_score[i]; by_size = i; }    // first maximum; NaN never wins
        }
    }
    if (lane == 0) {
        const float iou = (float)a.counts[0] / (float)a.counts[1];
        const float d = kd_distance(s_R[0], s_T[0], s_R[1], s_T[1]);
        bool create;
        if (!p.check_overlap) create = true;
        else if (K < p.window_size) create = iou < p.kf_overlap;
        else create = (iou < p.kf_overlap && d > p.kf_min_translation * median) || d > p.kf_translation * median;
        create = create && p.frames_since_last_kf >= p.kf_interval;
        a.out[0] = create ? 1u : 0u;
        a.out[1] = (uint32_t)cut;
        a.out[2] = (uint32_t)by_size;
        a.out[3] = __float_as_uint(iou);
        a.out[4] = __float_as_uint(d);
        a.out[5] = __float_as_uint(median);
        a.out[6] = 0u;
        a.out[7] = 0u;
    }
}

}  // namespace mgs

using namespace mgs;

extern "C" {

size_t mgs_median_scratch_bytes(uint64_t n) {
    return ((size_t)MD_HDR + (size_t)md_workgroups(n) * MD_BINS) * sizeof(uint32_t);
}

int mgs_masked_median(const float* values, const float* mask, uint64_t n, float lo, void* scratch, float* out_median,
                      uint32_t* out_count, void* stream) {
    if (n >= ((uint64_t)1 << 32)) { set_error("mgs_masked_median: n must stay below 2^32"); return 1; }
    if (lo != lo) { set_error("mgs_masked_median: lo must not be NaN"); return 1; }
    if (!scratch || !out_median || !out_count) {
        set_error("mgs_masked_median: scratch, out_median and out_count must be non-NULL");
        return 1;
    }
    if (n > 0 && !values) { set_error("mgs_masked_median: values must be non-NULL"); return 1; }
    uint32_t lo_bits;
    __builtin_memcpy(&lo_bits, &lo, sizeof(lo_bits));
    const uint32_t lo_key = md_key(lo_bits);
    const int G = (int)md_workgroups(n);
    const uint32_t* v = (const uint32_t*)values;
    const uint32_t* m = (const uint32_t*)mask;
    uint32_t* sc = (uint32_t*)scratch;
    hipStream_t s = (hipStream_t)stream;
    median_pass<0>(v, m, n, lo_key, sc, G, out_median, out_count, s);
    median_pass<1>(v, m, n, lo_key, sc, G, out_median, out_count, s);
    median_pass<2>(v, m, n, lo_key, sc, G, out_median, out_count, s);
    MGS_HIP(hipGetLastError());
    return 0;
}

int mgs_covisibility(int32_t P, const int32_t* cur_n_touched, const uint64_t* cur_bits, int32_t K,
                     const uint64_t* const* kf_bits, const uint64_t* kf_words, uint64_t* cur_bits_out, uint32_t* counts,
                     void* stream) {
    if (P < 0 || K < 0 || K > KW_MAX_KF) { set_error("mgs_covisibility: P >= 0 and 0..32 keyframes"); return 1; }
    if ((cur_n_touched != nullptr) == (cur_bits != nullptr)) {
        set_error("mgs_covisibility: exactly one of cur_n_touched and cur_bits must be given");
        return 1;
    }
    if (K > 0 && (!kf_bits || !kf_words || !counts)) {
        set_error("mgs_covisibility: kf_bits, kf_words and counts must be non-NULL");
        return 1;
    }
    CovisArgs a;
    const uint64_t words = ((uint64_t)P + 63) / 64;
    for (int k = 0; k < KW_MAX_KF; ++k) {
        const bool on = k < K;
        if (on && !kf_bits[k] && kf_words[k] > 0) { set_error("mgs_covisibility: NULL keyframe row"); return 1; }
        a.kf_bits[k] = on ? (const unsigned long long*)kf_bits[k] : nullptr;
        a.kf_words[k] = on ? (uint32_t)(kf_words[k] < words ? kf_words[k] : words) : 0u;
    }
    if (K == 0 || P == 0) return 0;
    a.cur_n_touched = cur_n_touched;
    a.cur_bits = (const unsigned long long*)cur_bits;
    a.cur_out = (unsigned long long*)cur_bits_out;
    a.counts = counts;
    a.K = K; a.P = P; a.words = (uint32_t)words;
    const uint64_t want = (words + 4 * CV_WAVES - 1) / (4 * CV_WAVES);
    const unsigned G = (unsigned)(want < 1 ? 1 : want > CV_MAX_WG ? CV_MAX_WG : want);
    hipStream_t s = (hipStream_t)stream;
    MGS_HIP(hipMemsetAsync(counts, 0, (size_t)K * 4 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(covisibility_kernel, dim3(G), dim3(CV_THREADS), 0, s, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

int mgs_keyframe_decide(const MgsKeyframeParams* params, const uint32_t* counts, const float* median,
                        const float* const* poses, uint32_t* out, void* stream) {
    if (!params || !counts || !median || !poses || !out) {
        set_error("mgs_keyframe_decide: params, counts, median, poses and out must be non-NULL");
        return 1;
    }
    if (params->K < 1 || params->K > KW_MAX_KF) { set_error("mgs_keyframe_decide: 1..32 window keyframes"); return 1; }
    if (params->window_size < 1 || params->n_dont_touch < 1) {
        set_error("mgs_keyframe_decide: window_size and n_dont_touch must be at least 1");
        return 1;
    }
    DecideArgs a;
    a.p = *params;
    a.counts = counts; a.median = median; a.out = out;
    for (int i = 0; i < KD_MAX; ++i) {
        const bool on = i <= params->K;
        if (on && (!poses[2 * i] || !poses[2 * i + 1])) { set_error("mgs_keyframe_decide: NULL pose pointer"); return 1; }
        a.R[i] = on ? poses[2 * i] : nullptr;
        a.T[i] = on ? poses[2 * i + 1] : nullptr;
    }
    hipLaunchKernelGGL(keyframe_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    MGS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
