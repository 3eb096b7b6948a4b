// kernels_bank.hpp -- a channel bank's bookkeeping around the tracking kernels: end of a speculative block, reset, small helpers.
// A part of kernels.hpp (which lists every kernel); the parts build on each other in the order kernels.hpp includes them.
#pragma once
#include "kernels_dll_exact.hpp"

namespace gyp {

// End of a block under the round protocol (one workgroup per channel, main stream, behind the last verify kernels): the reports of
// the last two rounds are consulted the way the tracking kernel would in two more rounds.  A channel whose every sub-block has
// held takes the exact code loop's final state; any other one is handed to the transform kernel (bad / bad_from), which restarts
// from ckpt[bad_from] -- where the channel never started that sub-block, its present state IS that checkpoint.
struct SpecFinalizeParams {
    SpecCtl* ctl;
    const int32_t* trk;
    const int32_t* fail;
    ChanState* states;
    ChanState* ckpt;
    const DllExact* hist;
    DllExact* exact;
    int32_t* bad;
    int32_t* bad_from;
    int32_t* stats;      // [4] += {-, -, sub-block re-dos, channels handed to the transform kernel}
    int32_t n_chan, n_sub, rounds;
};
__global__ __launch_bounds__(256) void spec_finalize_kernel(SpecFinalizeParams p) {
    const int ch = blockIdx.x;
    if (ch >= p.n_chan) return;
    __shared__ int s_copy_to;
    if (threadIdx.x == 0) {
        SpecCtl c = p.ctl[ch];
        for (int R = p.rounds; R < p.rounds + 2; ++R) {
            if (c.dead || R < 2 || c.rb_round == R - 1) continue;
            const int s = p.trk[(size_t)(R - 2) * p.n_chan + ch];
            if (s >= 0 && p.fail[(size_t)(R - 2) * p.n_chan + ch] != kNoFail) { c.dead = 1; c.cursor = s; }
        }
        const bool ok = !c.dead && c.cursor >= p.n_sub;
        p.bad[ch] = ok ? 0 : 1;
        p.bad_from[ch] = ok ? kNoFail : c.cursor;
        s_copy_to = -1;
        if (ok) {
            const DllExact x = p.hist[(size_t)p.n_sub * p.n_chan + ch];
            p.states[ch].dll_phase = x.dll; p.states[ch].code_phase = x.code_phase;
            p.exact[ch] = x;
        } else {
            atomicAdd(p.stats + 3, 1);
            if (!c.dead) s_copy_to = c.cursor;   // ran out of rounds in front of a sub-block it never started
        }
        if (c.redos) atomicAdd(p.stats + 2, c.redos);
        p.ctl[ch] = c;
    }
    __syncthreads();
    if (s_copy_to >= 0) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.states + ch);
        uint32_t* dst = reinterpret_cast<uint32_t*>(p.ckpt + (size_t)s_copy_to * p.n_chan + ch);
        for (int i = threadIdx.x; i < (int)(sizeof(ChanState) / 4); i += blockDim.x) dst[i] = src[i];
    }
}

// out[0] = how many of v[0 .. n) are non-zero (one wavefront)
__global__ void count_nonzero_kernel(const int32_t* __restrict__ v, int32_t n, int32_t* __restrict__ out) {
    int c = 0;
    for (int i = threadIdx.x; i < n; i += 64) c += v[i] != 0 ? 1 : 0;
    for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off, 64);
    if (threadIdx.x == 0) out[0] = c;
}
// {a, b, c, d} -> p[0..3] on the stream (telemetry headers: no host buffer has to outlive the call)
__global__ void set4_kernel(int32_t* p, int32_t a, int32_t b, int32_t c, int32_t d) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { p[0] = a; p[1] = b; p[2] = c; p[3] = d; }
}

__global__ void bank_reset_kernel(ChanState* states, const gyp_chan_init* inits, int n_chan) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chan) return;
    ChanState* s = states + i;
    const gyp_chan_init in = inits[i];
    s->stream = in.stream; s->sat_id = in.sat_id;
    s->doppler = in.doppler_hz; s->carrier_phase = in.carrier_phase;
    s->dll_phase = (double)in.code_phase;   // tracker.py:224
    s->last_watchdog_time = 0.0;
    s->n_steps = 0;
    s->code_phase = in.code_phase;
    s->lost = 0;
    s->win_centre1 = 0; s->pad0 = 0;
    s->sums = LockSums{};
}

}  // namespace gyp
