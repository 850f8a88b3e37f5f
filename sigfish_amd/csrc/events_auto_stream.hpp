// events_auto_stream.hpp -- the RNA automatic query start ("-p -1") of a raw-signal SESSION (sfa_session_raw_auto_start).
// The batch path (events_kernels.hpp, ev_autostart_*) runs detect_query_start once over a whole read; its adaptor segmenter is
// not causal (the threshold is mean - std_scale * sd of the rolling mean over the WHOLE signal), so a session has a rule of its
// own, stated on samples: target(N) = what detect_query_start computes before it looks at events (polya.y + ad.y, or -1),
// applied to a slot's first N samples, evaluated at the points N_k = k * every_samples <= max_samples and at one final point
// min(samples received, max_samples); the first point with target >= 0 freezes the slot's target.  CPU twin of target(N):
// sfa::auto_start_target (host/events.cpp); of the rule: tests/autostart_oracle.py.
//
// ev_auto_append_kernel: one block per entry of the call; the chunk's samples are appended to the slot's retention buffer
// (int16, max_samples per slot) from the staging the detector reads.  Samples beyond the cap are not kept.
// ev_auto_eval_kernel: one wave per entry that has a pending point.  The integer prefix sum S of the clamped samples is exact
// and does not depend on N, so it is computed once up to the entry's last point and every point reads its own prefix of it
// (the rolling mean is t[j] = (float)(S[j + 2000] - S[j]) / 2000, events_kernels.hpp:606-611).  Everything behind it is the
// reference's sequential fp32 arithmetic: all lanes stage a tile of the sequence into LDS, lane 0 walks it in order with the
// batch kernel's loops and early exits (restated here, the batch kernel is left as it is), the result is the host twin's bit
// for bit.  The points of an entry are taken in ascending order, each on its own prefix, until one gives a target.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "events_stream.hpp"
#include "jnn_consts.hpp"

namespace sfa {

struct EvAutoAppendArgs {
    const int16_t *raw;      // the call's samples (EvStreamArgs.raw)
    const int64_t *raw_off;  // [n + 1]
    const int32_t *slot;     // [n]
    const int32_t *e_flags;  // [n] kEntryFresh: the slot's automatic start is reset
    const int32_t *have;     // [n] samples the slot had received before this call
    int16_t *keep;           // [n_slots][max_samples]
    EvAutoSlot *state;       // [n_slots]
    int32_t n, max_samples;
};

__global__ void __launch_bounds__(256) ev_auto_append_kernel(const EvAutoAppendArgs a) {
    const int i = blockIdx.x;
    const int64_t b = a.raw_off[i];
    const int64_t len = a.raw_off[i + 1] - b;
    const int slot = a.slot[i];
    const int64_t have = a.have[i];
    if (threadIdx.x == 0 && (a.e_flags[i] & 1)) {  // kEntryFresh
        EvAutoSlot z;
        z.target = -1, z.skip = -1, z.frozen_at = 0, z.status = kAutoPending;
        a.state[slot] = z;
    }
    if (have >= a.max_samples) return;
    const int take = static_cast<int>(min(len, static_cast<int64_t>(a.max_samples) - have));  // have + take <= max_samples
    int16_t *dst = a.keep + static_cast<int64_t>(slot) * a.max_samples + have;
    const int16_t *src = a.raw + b;
    for (int j = threadIdx.x; j < take; j += 256) dst[j] = src[j];
}

struct EvAutoEntry {  // a slot of the call that has pending points: n0, n0 + every, ... (n_periodic of them), then n_final
    int32_t entry;       // index into the call's tables (slot, scale)
    int32_t n0, n_periodic;
    int32_t n_final;     // -1: the call brings no final point.  A periodic point equal to it is taken once, as the final point
};

struct EvAutoEvalArgs {
    const EvAutoEntry *entries;  // [n_entries]
    const int32_t *slot;         // [n] of the call
    const float *scale;          // [n][2] offset, raw_unit
    const int16_t *keep;         // [n_slots][max_samples]
    int32_t *csum;               // [n_entries][max_samples + 1] scratch: prefix sums of the clamped samples
    EvAutoSlot *state;           // [n_slots]
    int32_t n_entries, max_samples, every;
    int32_t lo;                  // shortest adaptor (AutoArgs.lo)
    float std_scale;
};

constexpr int kAutoTile = 2048;  // floats staged per tile: 8 KB of LDS

// A sequence of `len` floats, element j = gen(j), visited in order by lane 0: f(j, v) returns false to stop early.  All lanes
// stage a tile, lane 0 walks it; the block is one wave.
template <typename G, typename F>
__device__ __forceinline__ void wave_walk(float *tile, int len, G &&gen, F &&f) {
    const int lane = threadIdx.x;
    for (int base = 0; base < len; base += kAutoTile) {
        const int n = min(kAutoTile, len - base);
        for (int j = lane; j < n; j += 64) tile[j] = gen(base + j);
        __syncthreads();
        int go = 1;
        if (lane == 0)
            for (int j = 0; j < n; ++j)
                if (!f(base + j, tile[j])) {
                    go = 0;
                    break;
                }
        go = __shfl(go, 0);
        __syncthreads();
        if (!go) break;
    }
}

// target(N) of the samples raw[0, N) with their prefix sums S[0, N]: sfa::auto_start_target.  Block-uniform result.
__device__ __forceinline__ int32_t auto_target(float *tile, const int16_t *raw, const int32_t *S, int32_t N, float off, float unit, int32_t lo,
                                               float std_scale) {
    if (N <= kAdWindow) return -1;
    const int m = N - kAdWindow;
    auto tmean = [&](int j) { return static_cast<float>(S[j + kAdWindow] - S[j]) / 2000.0f; };
    // mean_f(t), stdv_f(t) (stat.h:17-44): fp32 accumulators, divided by the int count
    float s = 0.0f;
    wave_walk(tile, m, tmean, [&](int, float x) {
        s += x;
        return true;
    });
    const float mn = s / static_cast<float>(m);
    float s2 = 0.0f;
    wave_walk(tile, m, tmean, [&](int, float x) {
        s2 += (x - mn) * (x - mn);
        return true;
    });
    const float sd = sqrtf(s2 / static_cast<float>(m));
    const float bot = mn - (sd * std_scale);

    // jnnv2()'s segment loop (jnn.c:130-163) as ev_autostart_scan_kernel keeps it: the last segment and the answer
    bool begin = false, have = false, found = false;
    int st = 0, en = 0, bx = 0, by = 0, ax = 0, ay = 0;
    auto valid = [&](int x, int y) { return !(y - x > kAdHi || y - x < lo); };
    wave_walk(tile, m, tmean, [&](int j, float v) {
        if (v < bot && !begin) {
            st = j;
            begin = true;
        } else if (v < bot) {
            en = j;
        } else if (v > bot && begin) {
            if (have && st - by < kAdSegDist) {
                by = en;
            } else {
                if (have && valid(bx, by)) {
                    found = true;
                    ax = bx;
                    ay = by;
                }
                bx = st;
                by = en;
                have = true;
            }
            st = en = 0;
            begin = false;
        }
        if (!found && have && (begin ? st : j + 1) - by >= kAdSegDist && valid(bx, by)) {
            found = true;
            ax = bx;
            ay = by;
        }
        return !found;
    });
    if (!found && have && valid(bx, by)) {
        found = true;
        ax = bx;
        ay = by;
    }
    const int adx = __shfl(ax, 0) + kAdWindow / 2 - 1, ady = __shfl(ay, 0) + kAdWindow / 2 - 1;
    if (!__shfl(found ? 1 : 0, 0) || ady <= 0) return -1;  // (uniform from here on)

    // m_a = mean_f(pA[ad.x .. ad.y)); pA = ((float)raw + offset) * raw_unit, as event_single()
    float sa = 0.0f;
    wave_walk(tile, ady - adx, [&](int j) { return (static_cast<float>(raw[adx + j]) + off) * unit; },
              [&](int, float x) {
                  sa += x;
                  return true;
              });
    const float m_a = sa / static_cast<float>(ady - adx);
    const float top = (m_a + 30.0f) + 20.0f, pbot = (m_a + 30.0f) - 20.0f;

    // jnn_core() (jnn.c:191-279) over pA[ad.y .. N): the first segment, final once a second one exists or nothing can merge
    bool prev = false;
    int err = 0, prev_err = 0, c = 0, w = kPaCorrector, pst = 0, nseg = 0, fy = 0;
    wave_walk(tile, N - ady, [&](int j) { return (static_cast<float>(raw[ady + j]) + off) * unit; },
              [&](int j, float pa) {
                  const float x = pa > 1200.0f ? 1200.0f : (pa < 0.0f ? 0.0f : pa);
                  if (x < top && x > pbot) {
                      if (!prev) {
                          pst = j;
                          prev = true;
                      }
                      c++;
                      w++;
                      if (prev_err) prev_err = 0;
                      if (c >= kPaWindow && c >= w && !(c % w)) err--;
                  } else {
                      if (prev && err < kPaError) {
                          c++;
                          err++;
                          prev_err++;
                          if (c >= kPaWindow && c >= w && !(c % w)) err--;
                      } else if (prev && c >= kPaWindow) {
                          const int end = j - prev_err;
                          prev = false;
                          if (nseg > 0 && pst - fy < kPaSegDist) {
                              if (nseg == 1) fy = end;
                          } else {
                              if (nseg == 0) fy = end;
                              ++nseg;
                          }
                          c = err = prev_err = 0;
                      } else if (prev) {
                          prev = false;
                          c = err = prev_err = 0;
                      }
                  }
                  return !(nseg >= 2 || (nseg == 1 && (prev ? pst : j + 1) - fy >= kPaSegDist));
              });
    const int nseg0 = __shfl(nseg, 0), fy0 = __shfl(fy, 0);
    return (nseg0 > 0 && fy0 > 0) ? fy0 + ady : -1;
}

__global__ void __launch_bounds__(64) ev_auto_eval_kernel(const EvAutoEvalArgs a) {
    __shared__ float tile[kAutoTile];
    const int lane = threadIdx.x;
    const EvAutoEntry e = a.entries[blockIdx.x];
    const int slot = a.slot[e.entry];
    const float off = a.scale[2 * e.entry], unit = a.scale[2 * e.entry + 1];
    const int16_t *raw = a.keep + static_cast<int64_t>(slot) * a.max_samples;
    int32_t *S = a.csum + static_cast<int64_t>(blockIdx.x) * (static_cast<int64_t>(a.max_samples) + 1);
    const int n_last = max(e.n_final, e.n_periodic > 0 ? e.n0 + (e.n_periodic - 1) * a.every : 0);  // <= max_samples (host)

    // S[j] = sum of clamp(raw[0, j)): a wave-wide integer scan, 64 samples a step
    if (lane == 0) S[0] = 0;
    int carry = 0;
    for (int base = 0; base < n_last; base += 64) {
        const int j = base + lane;
        int s = 0;
        if (j < n_last) {
            const int r = raw[j];
            s = r > 1200 ? 1200 : (r < 0 ? 0 : r);  // clamp_outlier() on an integer-valued float
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(s, o);
            if (lane >= o) s += u;
        }
        if (j < n_last) S[j + 1] = carry + s;
        carry += __shfl(s, 63);
    }
    __syncthreads();  // the block's stores of S are visible to its loads below

    int32_t target = -1, at = 0;
    for (int p = 0; p < e.n_periodic && target < 0; ++p) {
        const int N = e.n0 + p * a.every;
        if (N == e.n_final) break;  // (ascending: nothing periodic lies behind the final point)
        target = auto_target(tile, raw, S, N, off, unit, a.lo, a.std_scale);
        at = N;
    }
    bool final_pt = false;
    if (target < 0 && e.n_final >= 0) {
        target = auto_target(tile, raw, S, e.n_final, off, unit, a.lo, a.std_scale);
        at = e.n_final;
        final_pt = true;
    }
    if (lane == 0 && (target >= 0 || final_pt)) {
        EvAutoSlot o;
        o.target = target;
        o.frozen_at = at;
        o.skip = target >= 0 ? -1 : kAutoFallback;  // no target at the final point: the fallback, at once
        o.status = (target >= 0 ? kAutoPending : kAutoNoTarget) | (final_pt ? kAutoAtFinal : 0);
        a.state[slot] = o;
    }
}

}  // namespace sfa
