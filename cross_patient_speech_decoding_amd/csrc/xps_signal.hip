// Per-bin high-gamma feature extraction of the realtime pipeline (realtime_sim/realtime_processing.py:10-164
// process_HG): common average reference -> one IIR/FIR band-pass per band with carried filter state -> RMS over
// (time, bands) per channel.  One launch per 20 ms bin; float64 like the reference (numpy / scipy.signal.lfilter).
//
// A bin is tiny (128 channels x 40 samples x ~8 bands): the kernel is latency-bound; what it buys is that the features
// are produced on the device, in one launch, next to the hipGraph-captured GRU step that consumes them.
//
// Arithmetic order follows the reference bit for bit where it is defined:
//  * CAR: np.mean(data[good], axis=0) = sequential sum over the good channels in index order, / count; data - avg
//  * lfilter: scipy's direct-form-II-transposed loop, coefficients normalised by a[0], NO fused multiply-add
//  * power: np.mean(np.square(y), axis=(1, 2)) over the contiguous (time, band) block of a channel = numpy's pairwise
//    summation (8 accumulators up to 128 elements, recursive halving above), / count, sqrt
#include "xps_common.h"

namespace {
constexpr int HG_MAXT = 2048, HG_MAXTAPS = 32;

// numpy's pairwise_sum (loops_utils.h.src) on a contiguous array
__device__ double np_pairwise_sum(const double* a, int n) {
#pragma clang fp contract(off)
    // explicit stack of (start, length) segments; the combine order of the recursion is res(left) + res(right), which an
    // in-order traversal with a value stack reproduces
    int seg_start[24], seg_len[24], seg_state[24];
    double val[24];
    int sp = 0, vp = 0;
    seg_start[0] = 0; seg_len[0] = n; seg_state[0] = 0; sp = 1;
    while (sp > 0) {
        const int s = seg_start[sp - 1], len = seg_len[sp - 1], st = seg_state[sp - 1];
        if (len <= 128) {
            double res;
            if (len < 8) {
                res = 0.0;
                for (int i = 0; i < len; ++i) res += a[s + i];
            } else {
                double r[8];
                for (int j = 0; j < 8; ++j) r[j] = a[s + j];
                int i;
                for (i = 8; i < len - (len % 8); i += 8)
                    for (int j = 0; j < 8; ++j) r[j] += a[s + i + j];
                res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (; i < len; ++i) res += a[s + i];
            }
            val[vp++] = res;
            --sp;
        } else if (st == 0) {                       // descend into the left half
            int n2 = len / 2;
            n2 -= n2 % 8;
            seg_state[sp - 1] = 1;
            seg_start[sp] = s; seg_len[sp] = n2; seg_state[sp] = 0; ++sp;
        } else if (st == 1) {                       // then the right half
            int n2 = len / 2;
            n2 -= n2 % 8;
            seg_state[sp - 1] = 2;
            seg_start[sp] = s + n2; seg_len[sp] = len - n2; seg_state[sp] = 0; ++sp;
        } else {                                    // combine
            const double right = val[--vp], left = val[--vp];
            val[vp++] = left + right;
            --sp;
        }
    }
    return val[0];
}

// one block = HG_CPB channels; thread -> (local channel, band)
constexpr int HG_CPB = 8;
__global__ void process_hg_kernel(const double* __restrict__ data, int C, int Tn, const unsigned char* __restrict__ good,
                                  const double* __restrict__ bcoef, const double* __restrict__ acoef, int bands, int taps,
                                  double* __restrict__ zi, int do_car, double* __restrict__ car_out,
                                  double* __restrict__ filtered, double* __restrict__ power) {
#pragma clang fp contract(off)
    __shared__ double avg[HG_MAXT];
    const int tid = threadIdx.x, nthr = blockDim.x;
    // 1. common average over the good channels (every block recomputes it: C x Tn doubles, L2-resident)
    if (do_car) {
        int ngood = 0;
        for (int c = 0; c < C; ++c) ngood += (!good || good[c]) ? 1 : 0;
        for (int t = tid; t < Tn; t += nthr) {
            double s = 0.0;
            for (int c = 0; c < C; ++c)
                if (!good || good[c]) s += data[(long long)c * Tn + t];
            avg[t] = s / (double)ngood;
        }
    } else {
        for (int t = tid; t < Tn; t += nthr) avg[t] = 0.0;
    }
    __syncthreads();
    const int c0 = blockIdx.x * HG_CPB;
    if (car_out)
        for (int i = tid; i < HG_CPB * Tn; i += nthr) {
            const int c = c0 + i / Tn, t = i % Tn;
            if (c < C) car_out[(long long)c * Tn + t] = do_car ? data[(long long)c * Tn + t] - avg[t] : data[(long long)c * Tn + t];
        }
    // 2. filters: thread (cl, band)
    const int cl = tid / bands, band = tid % bands;
    const int c = c0 + cl;
    if (bands > 0 && cl < HG_CPB && c < C) {
        double b[HG_MAXTAPS], a[HG_MAXTAPS], z[HG_MAXTAPS];
        const double a0 = acoef ? acoef[(long long)band * taps] : 1.0;
        for (int k = 0; k < taps; ++k) {
            b[k] = bcoef[(long long)band * taps + k] / a0;
            a[k] = acoef ? acoef[(long long)band * taps + k] / a0 : (k == 0 ? 1.0 : 0.0);
        }
        double* zp = zi ? zi + ((long long)band * C + c) * (taps - 1) : nullptr;
        for (int k = 0; k < taps - 1; ++k) z[k] = zp ? zp[k] : 0.0;
        const double* xr = data + (long long)c * Tn;
        double* yo = filtered + ((long long)c * Tn) * bands + band;
        for (int t = 0; t < Tn; ++t) {
            const double x = do_car ? xr[t] - avg[t] : xr[t];
            double y;
            if (taps > 1) {
                y = z[0] + b[0] * x;
                for (int k = 0; k < taps - 2; ++k) z[k] = z[k + 1] + x * b[k + 1] - y * a[k + 1];
                z[taps - 2] = x * b[taps - 1] - y * a[taps - 1];
            } else {
                y = x * b[0];
            }
            yo[(long long)t * bands] = y;
        }
        if (zp)
            for (int k = 0; k < taps - 1; ++k) zp[k] = z[k];
    }
    __syncthreads();
    // 3. RMS over the contiguous (time, band) block of each channel, numpy's summation order
    if (power && bands > 0 && tid < HG_CPB && c0 + tid < C) {
        double* blk = filtered + (long long)(c0 + tid) * Tn * bands;
        const int n = Tn * bands;
        for (int i = 0; i < n; ++i) blk[i] = blk[i] * blk[i];          // np.square (in place on the scratch copy)
        power[c0 + tid] = sqrt(np_pairwise_sum(blk, n) / (double)n);
    }
}
}  // namespace

extern "C" size_t xps_process_hg_f64_workspace(int C, int Tn, int bands) {
    if (C < 1 || Tn < 1 || bands < 1) return 16;
    return (size_t)C * Tn * bands * sizeof(double) + 16;
}

extern "C" int xps_process_hg_f64(const double* data, int C, int Tn, const uint8_t* good, const double* b, const double* a,
                                  int bands, int taps, double* zi, int do_car, double* car_out, double* filtered,
                                  double* power, void* workspace, size_t workspace_bytes, void* stream) {
    XPS_CHECK_ARG(data && C >= 1 && Tn >= 1 && bands >= 0, "bad argument");
    XPS_CHECK_ARG(Tn <= HG_MAXT, "bin longer than 2048 samples");
    XPS_CHECK_ARG(bands == 0 || (b && taps >= 1 && taps <= HG_MAXTAPS), "1..32 filter taps");
    XPS_CHECK_ARG(bands <= 32, "at most 32 bands");
    XPS_CHECK_ARG(!power || bands > 0, "band power needs at least one band");
    double* filt = filtered;
    if (bands > 0 && !filt) {                     // the squared copy lives in the workspace when the caller does not want y
        if (!workspace || workspace_bytes < xps_process_hg_f64_workspace(C, Tn, bands)) {
            xps_set_error("xps_process_hg_f64: workspace too small");
            return XPS_E_WORKSPACE;
        }
        filt = (double*)workspace;
    }
    XPS_CHECK_ARG(!(filtered && power), "ask for the filtered signal OR the band power in one call (the power pass squares in place)");
    const int threads = bands > 0 ? ((HG_CPB * bands + 63) / 64) * 64 : 64;
    hipLaunchKernelGGL(process_hg_kernel, dim3(cdiv(C, HG_CPB)), dim3(threads), 0, (hipStream_t)stream, data, C, Tn,
                       (const unsigned char*)good, b, a, bands, taps, zi, do_car, car_out, filt, power);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

// Multi-bin, multi-stream frontend of the realtime pipeline (realtime_sim/realtime_pipeline.py): k consecutive bins of
// n_streams streams in one launch; bin j of stream s is exactly process_HG(bins[s][j], filt_ics=<state after bin j-1>).
// Grid (C / HG_CPB, n_streams); a block walks the k bins in order and keeps its (channel, band) filter state in registers
// across them, so each recurrence runs sequentially over k x Tn samples.  Per bin the arithmetic is process_hg_kernel's:
// CAR summed in channel order, DF-II-transposed without fma, numpy's pairwise sum over the bin's own (Tn x bands) block.
// The squared filter output is written directly (y * y is the value np.square produces from the stored y).
// MAXT bounds the taps at compile time: the tap loops unroll with guards, so coefficients and state stay in registers.
namespace {
template <int MAXT>
__global__ __launch_bounds__(256) void pipe_frontend_kernel(const double* __restrict__ bins, int k, int C, int Tn,
                                     const unsigned char* __restrict__ good, const double* __restrict__ bcoef,
                                     const double* __restrict__ acoef, int bands, int taps, double* __restrict__ zi,
                                     double* __restrict__ sq, double* __restrict__ power) {
#pragma clang fp contract(off)
    __shared__ double avg[HG_MAXT];
    const int tid = threadIdx.x, nthr = blockDim.x, s = blockIdx.y;
    const int c0 = blockIdx.x * HG_CPB;
    const unsigned char* gs = good ? good + (long long)s * C : nullptr;
    int ngood = 0;
    for (int c = 0; c < C; ++c) ngood += (!gs || gs[c]) ? 1 : 0;
    const int cl = tid / bands, band = tid % bands;
    const int c = c0 + cl;
    const bool filt = cl < HG_CPB && c < C;
    double b[MAXT], a[MAXT], z[MAXT];
    double* zp = nullptr;
#pragma unroll
    for (int q = 0; q < MAXT; ++q) { b[q] = 0.0; a[q] = 0.0; z[q] = 0.0; }
    if (filt) {
        const double a0 = acoef ? acoef[(long long)band * taps] : 1.0;
#pragma unroll
        for (int q = 0; q < MAXT; ++q)
            if (q < taps) {
                b[q] = bcoef[(long long)band * taps + q] / a0;
                a[q] = acoef ? acoef[(long long)band * taps + q] / a0 : (q == 0 ? 1.0 : 0.0);
            }
        zp = zi ? zi + (((long long)s * bands + band) * C + c) * (taps - 1) : nullptr;
#pragma unroll
        for (int q = 0; q < MAXT - 1; ++q)
            if (q < taps - 1) z[q] = zp ? zp[q] : 0.0;
    }
    double* sblk = sq + (long long)s * C * Tn * bands;
    for (int j = 0; j < k; ++j) {
        const double* data = bins + ((long long)s * k + j) * C * Tn;
        // 1. common average over the good channels, in channel order
        for (int t = tid; t < Tn; t += nthr) {
            double acc = 0.0;
            for (int cc = 0; cc < C; ++cc)
                if (!gs || gs[cc]) acc += data[(long long)cc * Tn + t];
            avg[t] = acc / (double)ngood;
        }
        __syncthreads();
        // 2. filters; a FIR (zi == NULL) starts every bin from a zero state, as the reference does
        if (filt) {
            if (!zp) {
#pragma unroll
                for (int q = 0; q < MAXT; ++q) z[q] = 0.0;
            }
            const double* xr = data + (long long)c * Tn;
            double* yo = sblk + ((long long)c * Tn) * bands + band;
            for (int t = 0; t < Tn; ++t) {
                const double x = xr[t] - avg[t];
                double y;
                if (taps > 1) {
                    y = z[0] + b[0] * x;
                    // z[q] = z[q+1] + x b[q+1] - y a[q+1] for q < taps - 2, then z[taps-2] = x b[taps-1] - y a[taps-1]
#pragma unroll
                    for (int q = 0; q < MAXT - 1; ++q) {
                        if (q < taps - 2) z[q] = z[q + 1] + x * b[q + 1] - y * a[q + 1];
                        else if (q == taps - 2) z[q] = x * b[q + 1] - y * a[q + 1];
                    }
                } else {
                    y = x * b[0];
                }
                yo[(long long)t * bands] = y * y;
            }
        }
        __syncthreads();
        // 3. RMS over the channel's contiguous (time, band) block of this bin
        if (tid < HG_CPB && c0 + tid < C) {
            const int n = Tn * bands;
            power[((long long)s * k + j) * C + c0 + tid] = sqrt(np_pairwise_sum(sblk + (long long)(c0 + tid) * n, n) / (double)n);
        }
        __syncthreads();          // avg and the squared block are rewritten by the next bin
    }
    if (zp) {
#pragma unroll
        for (int q = 0; q < MAXT - 1; ++q)
            if (q < taps - 1) zp[q] = z[q];
    }
}
}  // namespace

extern "C" size_t xps_pipe_frontend_f64_workspace(int n_streams, int C, int Tn, int bands) {
    if (n_streams < 1 || C < 1 || Tn < 1 || bands < 1) return 16;
    return (size_t)n_streams * C * Tn * bands * sizeof(double) + 16;
}

extern "C" int xps_pipe_frontend_f64(const double* bins, int n_streams, int k, int C, int Tn, const uint8_t* good,
                                     const double* b, const double* a, int bands, int taps, double* zi, double* power,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    XPS_CHECK_ARG(bins && power && n_streams >= 1 && k >= 1 && C >= 1 && Tn >= 1, "bad argument");
    XPS_CHECK_ARG(n_streams <= 8, "1..8 streams per call");
    XPS_CHECK_ARG(Tn <= HG_MAXT, "bin longer than 2048 samples");
    XPS_CHECK_ARG(b && bands >= 1 && bands <= 32 && taps >= 1 && taps <= HG_MAXTAPS, "1..32 bands of 1..32 filter taps");
    XPS_CHECK_ARG(!zi || a, "a carried state needs IIR coefficients (a)");
    if (!workspace || workspace_bytes < xps_pipe_frontend_f64_workspace(n_streams, C, Tn, bands)) {
        xps_set_error("xps_pipe_frontend_f64: workspace too small");
        return XPS_E_WORKSPACE;
    }
    const int threads = ((HG_CPB * bands + 63) / 64) * 64;
#define LAUNCH(MT) hipLaunchKernelGGL(pipe_frontend_kernel<MT>, dim3(cdiv(C, HG_CPB), n_streams), dim3(threads), 0,      \
                                      (hipStream_t)stream, bins, k, C, Tn, (const unsigned char*)good, b, a, bands, taps, zi, \
                                      (double*)workspace, power);
    if (taps <= 9) { LAUNCH(9) }                  // band-pass IIR up to order 4
    else if (taps <= 17) { LAUNCH(17) }           // up to order 8
    else { LAUNCH(HG_MAXTAPS) }
#undef LAUNCH
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

// Session replay (realtime_sim/session_replay.py): the high-gamma power of N recorded trials in one launch, each trial bit
// for bit what xps_pipe_frontend_f64 gives a stream fed the trial's bins in order.  Grid (N, channel tiles); one workgroup
// owns a trial's tile of NT / bands channels for all its bins:
//   * the bin (C x Tn) is read from global memory once, widened to double and staged in LDS; with PF > 0 the next bin is
//     already on its way into registers while this one is filtered;
//   * the common average is summed from LDS in channel order by one lane per sample, then subtracted once per staged
//     sample of the tile (x - avg is the value every band of the channel filters);
//   * lane (channel, band) keeps coefficients and DF-II-transposed state in registers across the bins (EXACT: the tap
//     count is the template's, so the update unrolls without guards);
//   * FAST8 (bands == 8): element i = t * 8 + band of the channel's block, and every leaf of numpy's pairwise sum starts
//     at a multiple of 8, so accumulator r[band] of a leaf is the lane's own running sum over the leaf's samples.  The
//     leaf's ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) is three xor-exchanges among the channel's 8 lanes and the leaves meet
//     in recursion order on a small value stack kept as a shift register.  The leaf schedule depends on Tn alone and
//     comes from the host (HgSched).  Nothing squared touches memory;
//   * other band counts write y * y to the workspace and sum it with np_pairwise_sum, one lane per channel, as
//     pipe_frontend_kernel does.
// A bin that does not fit in LDS (staged == 0) is read from global memory by every consumer instead.
namespace {
struct HgSched {
    int n_leaves;
    unsigned char rows[256];      // samples (rows of 8 elements) of leaf i: at most 16
    unsigned char pops[256];      // left + right combinations that follow leaf i
};
constexpr int HG_STACK = 10;      // depth of the combination stack: Tn <= 2048 -> at most 256 leaves, 9 levels

void hg_sched_rec(int m, HgSched& s) {
    if (m <= 16) {                // numpy's leaf: n = 8 m <= 128 elements
        s.rows[s.n_leaves] = (unsigned char)m;
        s.pops[s.n_leaves] = 0;
        ++s.n_leaves;
        return;
    }
    const int m2 = m / 2;         // n2 = n / 2, n2 -= n2 % 8 in units of 8 elements
    hg_sched_rec(m2, s);
    hg_sched_rec(m - m2, s);
    ++s.pops[s.n_leaves - 1];
}

template <int MAXT, bool EXACT, bool FAST8, int NT, int PF>
__global__ __launch_bounds__(NT) void hg_trials_kernel(
        const void* __restrict__ raw, int raw_is_f32, int n_bins, int C, int Tn, const long long* __restrict__ bins_per_trial,
        const unsigned char* __restrict__ good, int good_per_trial, const double* __restrict__ bcoef,
        const double* __restrict__ acoef, int bands_rt, int taps_rt, const double* __restrict__ zi0, int zi_per_trial,
        double* __restrict__ zi_out, double* __restrict__ power, double* __restrict__ sq, int staged, HgSched sched) {
#pragma clang fp contract(off)
    extern __shared__ double hg_lds[];
    double* avg = hg_lds;                         // [Tn]
    double* xs = hg_lds + Tn;                     // [C][Tn] when staged
    const int bands = FAST8 ? 8 : bands_rt;
    const int taps = EXACT ? MAXT : taps_rt;
    const int tid = threadIdx.x;
    const long long n = blockIdx.x;
    const int CT = NT / bands;
    const int c0 = blockIdx.y * CT;               // < C by the grid
    const int tileC = min(CT, C - c0);
    const int cl = tid / bands, band = tid % bands;
    const int c = c0 + cl;
    const bool filt = cl < tileC;
    const int cs = filt ? c : c0;                 // idle lanes read a row that exists
    const unsigned char* gs = good ? good + (good_per_trial ? n * C : 0) : nullptr;
    int ngood = 0;
    for (int cc = 0; cc < C; ++cc) ngood += (!gs || gs[cc]) ? 1 : 0;
    int Ln = n_bins;
    if (bins_per_trial) {
        const long long l = bins_per_trial[n];
        Ln = l < 0 ? 0 : (l > n_bins ? n_bins : (int)l);
    }
    const bool carry = acoef != nullptr;          // a FIR starts every bin from a zero state

    double b[MAXT], a[MAXT], z[MAXT];
#pragma unroll
    for (int q = 0; q < MAXT; ++q) { b[q] = 0.0; a[q] = 0.0; z[q] = 0.0; }
    if (filt) {
        const double a0 = acoef ? acoef[(long long)band * taps] : 1.0;
#pragma unroll
        for (int q = 0; q < MAXT; ++q)
            if (q < taps) {
                b[q] = bcoef[(long long)band * taps + q] / a0;
                a[q] = acoef ? acoef[(long long)band * taps + q] / a0 : (q == 0 ? 1.0 : 0.0);
            }
        if (carry && zi0) {
            const double* zp = zi0 + (((zi_per_trial ? n : 0) * bands + band) * C + c) * (long long)(taps - 1);
#pragma unroll
            for (int q = 0; q < MAXT - 1; ++q)
                if (q < taps - 1) z[q] = zp[q];
        }
    }

    const long long bin_elems = (long long)C * Tn;
    const long long trial_base = n * n_bins * bin_elems;
    const float* raw32 = (const float*)raw;
    const double* raw64 = (const double*)raw;
#define HG_LD(idx) (raw_is_f32 ? (double)raw32[(idx)] : raw64[(idx)])
    double pf[PF > 0 ? PF : 1];
    if (PF > 0 && Ln > 0) {
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            const long long i = tid + (long long)q * NT;
            pf[q] = i < bin_elems ? HG_LD(trial_base + i) : 0.0;
        }
    }
    const int nel = Tn * bands;
    double* sblk = FAST8 ? nullptr : sq + n * bin_elems * bands;

    for (int j = 0; j < Ln; ++j) {
        const long long base = trial_base + (long long)j * bin_elems;
        // 1. stage the bin
        if (staged) {
            if (PF > 0) {
#pragma unroll
                for (int q = 0; q < PF; ++q) {
                    const long long i = tid + (long long)q * NT;
                    if (i < bin_elems) xs[i] = pf[q];
                }
            } else {
                for (long long i = tid; i < bin_elems; i += NT) xs[i] = HG_LD(base + i);
            }
        }
        __syncthreads();
        if (PF > 0 && j + 1 < Ln) {
#pragma unroll
            for (int q = 0; q < PF; ++q) {
                const long long i = tid + (long long)q * NT;
                pf[q] = i < bin_elems ? HG_LD(base + bin_elems + i) : 0.0;
            }
        }
        // 2. common average over the good channels, in channel order
        for (int t = tid; t < Tn; t += NT) {
            double acc = 0.0;
            if (staged) {
                for (int cc = 0; cc < C; ++cc)
                    if (!gs || gs[cc]) acc += xs[(long long)cc * Tn + t];
            } else {
                for (int cc = 0; cc < C; ++cc)
                    if (!gs || gs[cc]) acc += HG_LD(base + (long long)cc * Tn + t);
            }
            avg[t] = acc / (double)ngood;
        }
        __syncthreads();
        if (staged) {                             // x - avg once per sample of the tile
            const int te = tileC * Tn;
            double* xt = xs + (long long)c0 * Tn;
            for (int i = tid; i < te; i += NT) xt[i] = xt[i] - avg[i % Tn];
            __syncthreads();
        }
        // 3. filters
        if (!carry) {
#pragma unroll
            for (int q = 0; q < MAXT; ++q) z[q] = 0.0;
        }
        const double* xr = xs + (long long)cs * Tn;
        const long long xg = base + (long long)cs * Tn;
#define HG_STEP(t_)                                                                                     \
        const double x = staged ? xr[(t_)] : HG_LD(xg + (t_)) - avg[(t_)];                              \
        double y;                                                                                       \
        if (taps > 1) {                                                                                 \
            y = z[0] + b[0] * x;                                                                        \
            _Pragma("unroll") for (int q = 0; q < MAXT - 1; ++q) {                                      \
                if (q < taps - 2) z[q] = z[q + 1] + x * b[q + 1] - y * a[q + 1];                        \
                else if (q == taps - 2) z[q] = x * b[q + 1] - y * a[q + 1];                             \
            }                                                                                           \
        } else {                                                                                        \
            y = x * b[0];                                                                               \
        }
        if (FAST8) {
            double st[HG_STACK];
#pragma unroll
            for (int q = 0; q < HG_STACK; ++q) st[q] = 0.0;
            int t = 0;
            for (int leaf = 0; leaf < sched.n_leaves; ++leaf) {
                const int rows = sched.rows[leaf];
                double r = 0.0;                   // 0 + y*y is y*y exactly: the leaf's r[band] = a[band] start
                for (int rr = 0; rr < rows; ++rr, ++t) {
                    HG_STEP(t)
                    r = r + y * y;
                }
                r = r + __shfl_xor(r, 1);
                r = r + __shfl_xor(r, 2);
                r = r + __shfl_xor(r, 4);
#pragma unroll
                for (int q = HG_STACK - 1; q > 0; --q) st[q] = st[q - 1];
                st[0] = r;
                for (int p = sched.pops[leaf]; p > 0; --p) {
                    st[0] = st[1] + st[0];        // left + right
#pragma unroll
                    for (int q = 1; q < HG_STACK - 1; ++q) st[q] = st[q + 1];
                }
            }
            if (filt && band == 0) power[(n * n_bins + j) * C + c] = sqrt(st[0] / (double)nel);
        } else {
            double* yo = sblk + ((long long)cs * Tn) * bands + band;
            for (int t = 0; t < Tn; ++t) {
                HG_STEP(t)
                if (filt) yo[(long long)t * bands] = y * y;
            }
            __syncthreads();
            if (tid < tileC)
                power[(n * n_bins + j) * C + c0 + tid] = sqrt(np_pairwise_sum(sblk + (long long)(c0 + tid) * nel, nel) / (double)nel);
        }
#undef HG_STEP
        __syncthreads();                          // avg, xs and the squared block are rewritten by the next bin
    }
#undef HG_LD
    if (zi_out && carry && filt) {
        double* zo = zi_out + ((n * bands + band) * C + c) * (long long)(taps - 1);
#pragma unroll
        for (int q = 0; q < MAXT - 1; ++q)
            if (q < taps - 1) zo[q] = z[q];
    }
    // rows past the trial's length are zeros
    const long long pad = (long long)(n_bins - Ln) * tileC;
    for (long long i = tid; i < pad; i += NT)
        power[(n * n_bins + Ln + i / tileC) * C + c0 + (int)(i % tileC)] = 0.0;
}

// features[n][j][:] = float32(power[n][j] @ W[m] + c[m]), m = map_of_trial[n]: window_shift_kernel's sum (channel order,
// one rounding to float32 at the end), so a replayed frame has the bits of the frame the pipeline puts in its window.
// Rows past a trial's length are zeros; a map index outside 0 .. n_maps - 1 gives NaN (also under the identity map)
// instead of a read out of bounds.
__global__ __launch_bounds__(256) void hg_features_kernel(const double* __restrict__ power, long long total, int n_bins, int C,
                                                          const long long* __restrict__ bins_per_trial,
                                                          const double* __restrict__ W, const double* __restrict__ cvec,
                                                          const int* __restrict__ map_of_trial, int n_maps, int d,
                                                          float* __restrict__ features) {
#pragma clang fp contract(fast)       // the build's default, stated: acc += p * w is one fma, as in window_shift_kernel
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const long long row = q / d;
        const int e = (int)(q % d);
        const long long n = row / n_bins;
        const int j = (int)(row % n_bins);
        float v;
        if (bins_per_trial && j >= bins_per_trial[n]) {
            v = 0.0f;
        } else {
            const double* p = power + row * C;
            const int m = map_of_trial ? map_of_trial[n] : 0;
            if (map_of_trial && (m < 0 || m >= n_maps)) {
                v = __builtin_nanf("");
            } else if (W) {
                const double* w = W + (long long)m * C * d + e;
                double acc = 0.0;
                for (int i = 0; i < C; ++i) acc += p[i] * w[(long long)i * d];
                if (cvec) acc += cvec[(long long)m * d + e];
                v = (float)acc;
            } else {
                v = (float)p[e];
            }
        }
        features[q] = v;
    }
}

constexpr size_t HG_LDS_MAX = 65536;              // static + dynamic LDS a launch gets without an attribute
inline size_t hg_align16(size_t v) { return (v + 15) & ~(size_t)15; }
}  // namespace

extern "C" size_t xps_hg_trials_f64_workspace(int64_t N, int n_bins, int C, int Tn, int bands) {
    if (N < 1 || n_bins < 1 || C < 1 || Tn < 1 || bands < 1) return 16;
    size_t bytes = hg_align16((size_t)N * n_bins * C * sizeof(double));       // the power when the caller keeps only features
    if (bands != 8) bytes += hg_align16((size_t)N * C * Tn * bands * sizeof(double));   // squared block of one bin per trial
    return bytes + 16;
}

extern "C" int xps_hg_trials_f64(const void* raw, int raw_is_f32, int64_t N, int n_bins, int C, int Tn,
                                 const int64_t* bins_per_trial, const uint8_t* good, int good_per_trial, const double* b,
                                 const double* a, int bands, int taps, const double* zi0, int zi_per_trial, double* zi_out,
                                 double* power, const double* W, const double* c, const int32_t* map_of_trial, int n_maps,
                                 int d, float* features, void* workspace, size_t workspace_bytes, void* stream) {
    XPS_CHECK_ARG(raw && N >= 1 && n_bins >= 1 && C >= 1 && Tn >= 1, "bad argument");
    XPS_CHECK_ARG(N <= 2147483647LL, "at most 2^31 - 1 trials per launch");
    XPS_CHECK_ARG(Tn <= HG_MAXT, "bin longer than 2048 samples");
    XPS_CHECK_ARG(b, "bad argument");
    XPS_CHECK_ARG(bands >= 1 && bands <= 32, "1..32 bands");
    XPS_CHECK_ARG(taps >= 1 && taps <= HG_MAXTAPS, "1..32 filter taps");
    XPS_CHECK_ARG(a || (!zi0 && !zi_out), "a carried state needs IIR coefficients (a)");
    XPS_CHECK_ARG(power || features, "nothing to compute: power and features are both NULL");
    XPS_CHECK_ARG((!W && !features) || d >= 1, "a feature map needs d >= 1");
    if (features) {
        XPS_CHECK_ARG(W || d == C, "the identity map needs d == C");
        XPS_CHECK_ARG(!W || n_maps >= 1, "a feature map needs n_maps >= 1");
        XPS_CHECK_ARG(!map_of_trial || n_maps >= 1, "map_of_trial needs n_maps >= 1");
    }
    if (!workspace || workspace_bytes < xps_hg_trials_f64_workspace(N, n_bins, C, Tn, bands)) {
        xps_set_error("xps_hg_trials_f64: workspace too small");
        return XPS_E_WORKSPACE;
    }
    const size_t pbytes = hg_align16((size_t)N * n_bins * C * sizeof(double));
    double* pw = power ? power : (double*)workspace;
    double* sq = (double*)((char*)workspace + pbytes);
    const bool fast8 = bands == 8;
    HgSched sched;
    sched.n_leaves = 0;
    if (fast8) hg_sched_rec(Tn, sched);
    const size_t lds_avg = (size_t)Tn * sizeof(double), lds_bin = (size_t)C * Tn * sizeof(double);
    const int staged = lds_avg + lds_bin <= HG_LDS_MAX ? 1 : 0;
    const size_t lds = lds_avg + (staged ? lds_bin : 0);
    const long long bin_elems = (long long)C * Tn;
#define LAUNCH(MT, EX, F8, NT, PF)                                                                                          \
    hipLaunchKernelGGL((hg_trials_kernel<MT, EX, F8, NT, PF>), dim3((unsigned)N, cdiv(C, NT / bands)), dim3(NT), lds,      \
                       (hipStream_t)stream, raw, raw_is_f32, n_bins, C, Tn, (const long long*)bins_per_trial,               \
                       (const unsigned char*)good, good_per_trial, b, a, bands, taps, zi0, zi_per_trial, zi_out, pw, sq,    \
                       staged, sched);
    // 1024 lanes hold a trial's 128 channels x 8 bands at 9 taps in 128 registers each; more taps, and the general path's
    // summation, take fewer lanes per workgroup.  The register prefetch covers a bin of up to 5 x 1024 samples (128 x 40).
    if (fast8 && taps <= 9) {
        const bool pf = staged && bin_elems <= 5LL * 1024;
        if (taps == 9) { if (pf) { LAUNCH(9, true, true, 1024, 5) } else { LAUNCH(9, true, true, 1024, 0) } }
        else { if (pf) { LAUNCH(9, false, true, 1024, 5) } else { LAUNCH(9, false, true, 1024, 0) } }
    } else if (fast8) {
        if (taps <= 17) { LAUNCH(17, false, true, 512, 0) } else { LAUNCH(HG_MAXTAPS, false, true, 256, 0) }
    } else {
        if (taps <= 9) { LAUNCH(9, false, false, 256, 0) }
        else if (taps <= 17) { LAUNCH(17, false, false, 256, 0) }
        else { LAUNCH(HG_MAXTAPS, false, false, 256, 0) }
    }
#undef LAUNCH
    XPS_CHECK_LAUNCH();
    if (features) {
        const long long total = (long long)N * n_bins * d;
        const long long blocks = (total + 255) / 256;
        hipLaunchKernelGGL(hg_features_kernel, dim3((unsigned)(blocks < 1048576 ? blocks : 1048576)), dim3(256), 0,
                           (hipStream_t)stream, pw, total, n_bins, C, (const long long*)bins_per_trial, W, c,
                           (const int*)map_of_trial, n_maps, d, features);
        XPS_CHECK_LAUNCH();
    }
    return XPS_OK;
}
