// Sample-rate conversion ahead of the feature front-end (nb_asr_amd/frontend.py Resampler / ResamplerStream): band-limited sinc
// interpolation with a Hann window, the definition of include/nbasr.h "resampler" and DESIGN.md 9.  With o = orig / gcd, n = new / gcd:
//
//     y[j] = sum over m of h[j mod n][m - (j / n) o - lo(j mod n)] * x[m],      |m n - j o| <= reach,  0 <= m < length
//
// reach is the largest integer d with d * min(o, n) * 99 < 600 o n, so the support is decided in integers and host, model and kernel
// agree on it; lo(p) = ceil((p o - reach) / n).  The coefficients arrive as a table of n phases with an odd row pitch (computed in
// float64 on the host, rounded once to float32).
//
// One thread computes one output sample: a single accumulator, its taps in ascending m, fmaf -- so an output's bits are a function of
// the utterance's samples alone, whatever the push sizes, the sample's place in the launch or the batch.  A stream's samples are read
// by absolute index from the retained tail or this push's samples (the Samples::at of sample_tail.h); the host decides which
// outputs a step computes (frontend.py: resample_final / resample_total / resample_retain_from) and the step refuses outputs whose
// samples the stream does not hold.  One more workgroup per utterance copies what the next push needs into the OTHER tail.
//
// The phase table lives in LDS when n <= 256 phases (a workgroup of 256 consecutive outputs then reads every row 256 / n times;
// the odd pitch spreads consecutive phases over the banks) and fits 32 KB; with more phases than threads no row is read twice by a
// workgroup, and the rows are read from global memory (the whole table is at most 200 KB and stays in the caches).
#include "sample_tail.h"

namespace nbasr {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxPhases = 1024;                 // reduced new rate (11 025 -> 16 000 has 640, 16 000 -> 44 100 has 441)
constexpr int kMaxRatio = 1024;                  // reduced original rate
constexpr int kMaxTaps = 48;                     // largest support (48 000 -> 16 000 has 37)
constexpr int kLdsFloats = 8192;                 // table in LDS up to 32 KB

struct Geometry {                                // of one pair of rates, all integers
    int o, n, reach, taps, pitch;
};

inline long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline long long m_lo(const Geometry& g, long long j) { return -floor_div(g.reach - j * g.o, g.n); }      // ceil((j o - reach) / n)
inline long long m_hi(const Geometry& g, long long j) { return floor_div(j * g.o + g.reach, g.n); }

int gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// 0 on success; the rates' reduced geometry in *g
int geometry(const char* who, int orig_freq, int new_freq, Geometry* g)
{
    NBASR_REQUIRE(orig_freq > 0 && new_freq > 0, NBASR_EINVAL, "%s: the rates must be positive (got %d -> %d)", who, orig_freq, new_freq);
    const int d = gcd(orig_freq, new_freq);
    g->o = orig_freq / d;
    g->n = new_freq / d;
    NBASR_REQUIRE(g->o <= kMaxRatio && g->n <= kMaxPhases, NBASR_EINVAL,
                  "%s: %d -> %d reduces to %d : %d, the limits are %d : %d", who, orig_freq, new_freq, g->o, g->n, kMaxRatio, kMaxPhases);
    const long long on = static_cast<long long>(g->o) * g->n;
    g->reach = static_cast<int>((600 * on - 1) / (99LL * (g->o < g->n ? g->o : g->n)));
    g->taps = 0;
    for (int p = 0; p < g->n; ++p) {
        const int t = static_cast<int>(m_hi(*g, p) - m_lo(*g, p) + 1);
        if (t > g->taps) g->taps = t;
    }
    NBASR_REQUIRE(g->taps <= kMaxTaps, NBASR_EINVAL, "%s: %d -> %d has a support of %d taps, the limit is %d", who, orig_freq, new_freq,
                  g->taps, kMaxTaps);
    g->pitch = g->taps | 1;
    return NBASR_OK;
}

// outputs first_out .. first_out + n_out - 1 of every utterance, first_out = k0 n + p0 (0 <= p0 < n); lengths (or NULL): utterance b
// has lengths[b] samples -- it reads nothing at or beyond them, and outputs at or beyond ceil(n lengths[b] / o) are written as zero
__global__ __launch_bounds__(kThreads) void resample_kernel(
    const float* __restrict__ tail_in, int tail_len, long long tail_first, int tail_ld, const float* __restrict__ wave, int n_new, int ld_wave,
    float* __restrict__ tail_out, int tail_out_first_rel, const float* __restrict__ table, int o, int n, int reach, int pitch, int use_lds,
    float* __restrict__ out, int ld_out, int col0, long long k0, int p0, int n_out, long long total_len, const int* __restrict__ lengths,
    int n_blocks)
{
    extern __shared__ float lds_table[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Samples src{tail_in + static_cast<size_t>(b) * tail_ld, wave + static_cast<size_t>(b) * ld_wave, tail_first, tail_len, n_new};

    if (static_cast<int>(blockIdx.x) == n_blocks) {   // the trailing workgroup: what the next push still needs
        const int out_len = tail_len + n_new - tail_out_first_rel;
        float4* __restrict__ dst = reinterpret_cast<float4*>(tail_out + static_cast<size_t>(b) * tail_ld);
        for (int q = tid; q < tail_ld / 4; q += kThreads) {
            float v[4];
            for (int c = 0; c < 4; ++c) v[c] = 4 * q + c < out_len ? src.at(tail_first + tail_out_first_rel + 4 * q + c) : 0.f;
            dst[q] = make_float4(v[0], v[1], v[2], v[3]);
        }
        return;
    }

    if (use_lds) {
        for (int i = tid; i < n * pitch; i += kThreads) lds_table[i] = table[i];
        __syncthreads();
    }
    const int t = blockIdx.x * kThreads + tid;
    if (t >= n_out) return;
    const unsigned at_phase = static_cast<unsigned>(p0) + static_cast<unsigned>(t);      // j = k0 n + at_phase (< 2^31 + n: 32-bit division)
    const long long k = k0 + at_phase / static_cast<unsigned>(n);
    const int p = static_cast<int>(at_phase % static_cast<unsigned>(n));
    const long long length = lengths ? lengths[b] : total_len;
    const long long j = k * n + p;
    float acc = 0.f;
    if (j * o < length * n) {                                                // j < ceil(n length / o)
        const int a = p * o - reach;
        const int lo = a >= 0 ? (a + n - 1) / n : -((-a) / n);               // ceil(a / n)
        const int hi = (p * o + reach) / n;
        const long long base = k * o + lo;                                   // the sample of the row's first coefficient
        const int i0 = base < 0 ? static_cast<int>(-base) : 0;
        const long long last = k * o + hi < length - 1 ? k * o + hi : length - 1;
        const int i1 = static_cast<int>(last - base);                        // taps i0 .. i1 of the row, ascending m
        if (use_lds) {
            const float* row = lds_table + p * pitch;
            for (int i = i0; i <= i1; ++i) acc = __builtin_fmaf(row[i], src.at(base + i), acc);
        } else {
            const float* __restrict__ row = table + p * pitch;
            for (int i = i0; i <= i1; ++i) acc = __builtin_fmaf(row[i], src.at(base + i), acc);
        }
    }
    out[static_cast<size_t>(b) * ld_out + col0 + t] = acc;
}

int launch(const char* who, const Geometry& g, const float* tail_in, int tail_len, long long tail_first, int tail_ld, const float* wave,
           int n_new, int ld_wave, float* tail_out, int tail_out_first_rel, const float* table, float* out, int ld_out, int col0,
           long long first_out, int n_out, long long total_len, const int* lengths, int batch, bool retain, nbasr_stream_t stream)
{
    const int n_blocks = (n_out + kThreads - 1) / kThreads;
    const int use_lds = g.n <= kThreads && g.n * g.pitch <= kLdsFloats;
    const size_t lds_bytes = use_lds ? static_cast<size_t>(g.n) * g.pitch * sizeof(float) : 0;
    hipLaunchKernelGGL(resample_kernel, dim3(n_blocks + (retain ? 1 : 0), batch), dim3(kThreads), lds_bytes, as_stream(stream), tail_in,
                       tail_len, tail_first, tail_ld, wave, n_new, ld_wave, tail_out, tail_out_first_rel, table, g.o, g.n, g.reach, g.pitch,
                       use_lds, out, ld_out, col0, first_out / g.n, static_cast<int>(first_out % g.n), n_out, total_len, lengths, n_blocks);
    return launch_status(who);
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_resample_state_bytes(int batch, int tail_capacity)
{
    if (batch <= 0 || tail_capacity <= 0) return 0;
    return static_cast<size_t>(2) * batch * ((tail_capacity + 3) / 4 * 4) * sizeof(float);
}

extern "C" int nbasr_resample_stream_step(const float* tail_in, int tail_len, long long tail_first, const float* wave, int n_new, int ld_wave,
                                          float* tail_out, int tail_out_first_rel, int tail_capacity, const float* table, int orig_freq,
                                          int new_freq, float* out, int ld_out, int col0, long long first_out, int n_out,
                                          long long total_len, int final, int batch, nbasr_stream_t stream)
{
    static const char* who = "nbasr_resample_stream_step";
    clear_error();
    Geometry g;
    if (const int rc = geometry(who, orig_freq, new_freq, &g)) return rc;
    NBASR_REQUIRE(tail_capacity > 0, NBASR_EINVAL, "%s: tail_capacity=%d must be positive", who, tail_capacity);
    const int tail_ld = (tail_capacity + 3) / 4 * 4;
    if (const int rc = tail_step_sizes(who, tail_ld, batch, tail_len, tail_first, n_new, ld_wave, first_out >= 0 && n_out >= 0 && col0 >= 0,
                                       total_len)) return rc;
    const bool retain = !final && tail_out != nullptr;
    if (batch == 0 || (n_out == 0 && (n_new == 0 || !retain))) return NBASR_OK;
    if (const int rc = tail_step_pointers(who, batch, tail_in, tail_len, wave, n_new)) return rc;
    if (n_out > 0) {
        NBASR_REQUIRE(table && out, NBASR_ENULL, "%s: NULL pointer", who);
        NBASR_REQUIRE(col0 + static_cast<long long>(n_out) <= ld_out, NBASR_EINVAL, "%s: columns %d..%lld do not fit ld_out=%d", who, col0,
                      col0 + static_cast<long long>(n_out) - 1, ld_out);
        // every sample the outputs touch must be in [tail_first, total_len); beyond the end only once the end is known
        const long long last_out = first_out + n_out - 1;
        long long lo = m_lo(g, first_out), top = m_hi(g, last_out);
        if (lo < 0) lo = 0;
        if (final) {
            NBASR_REQUIRE(last_out * g.o < total_len * g.n, NBASR_EINVAL, "%s: output %lld is beyond the %lld outputs of %lld samples", who,
                          last_out, (total_len * g.n + g.o - 1) / g.o, total_len);
            if (top >= total_len) top = total_len - 1;
        }
        NBASR_REQUIRE(lo >= tail_first && top < total_len, NBASR_EINVAL, "%s: outputs %lld..%lld need samples %lld..%lld, the stream holds %lld..%lld",
                      who, first_out, last_out, lo, top, tail_first, total_len - 1);
    }
    if (retain)
        if (const int rc = tail_step_retain(who, tail_ld, tail_in, tail_len, n_new, tail_out, tail_out_first_rel)) return rc;
    return launch(who, g, tail_in, tail_len, tail_first, tail_ld, wave, n_new, ld_wave, tail_out, tail_out_first_rel, table, out, ld_out, col0,
                  first_out, n_out, total_len, nullptr, batch, retain, stream);
}

extern "C" int nbasr_resample(const float* wave, int ld_wave, int samples, const int* lengths, const float* table, int orig_freq, int new_freq,
                              float* out, int ld_out, int n_out, int batch, nbasr_stream_t stream)
{
    static const char* who = "nbasr_resample";
    clear_error();
    Geometry g;
    if (const int rc = geometry(who, orig_freq, new_freq, &g)) return rc;
    NBASR_REQUIRE(batch >= 0 && samples >= 0 && ld_wave >= samples && n_out >= 0, NBASR_EINVAL, "%s: bad sizes", who);
    const long long want = (static_cast<long long>(samples) * g.n + g.o - 1) / g.o;
    NBASR_REQUIRE(n_out == want, NBASR_EINVAL, "%s: %d samples at %d -> %d make %lld outputs, not %d", who, samples, orig_freq, new_freq, want,
                  n_out);
    NBASR_REQUIRE(ld_out >= n_out, NBASR_EINVAL, "%s: %d outputs do not fit ld_out=%d", who, n_out, ld_out);
    if (batch == 0 || n_out == 0) return NBASR_OK;
    NBASR_REQUIRE(batch <= 65535, NBASR_EINVAL, "%s: batch %d > 65535", who, batch);
    NBASR_REQUIRE(wave && table && out, NBASR_ENULL, "%s: NULL pointer", who);
    // the stream step with an empty tail and the end known: lengths[b] <= samples is the caller's to keep (device memory)
    return launch(who, g, wave, 0, 0, 0, wave, samples, ld_wave, nullptr, 0, table, out, ld_out, 0, 0, n_out, samples, lengths, batch, false,
                  stream);
}
