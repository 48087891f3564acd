// Per-token confidence over CTC logits (nb_asr_amd.ctc confidence / ConfidenceStream): the definition of include/nbasr.h "confidence"
// and DESIGN.md 9 "Confidence".  A frame's softmax becomes one number in [0, 1] (the probability of its label, or the normalised Gibbs or
// Tsallis entropy of Laptev and Ginsburg), quantised at once to q = rint(conf * 2^24); a token -- a maximal run of one non-blank label --
// records the minimum and the 64-bit sum of its frames' q.  Everything after the quantisation is integer arithmetic, so whole = chunked
// = peeked = a row alone, to the bit, whatever frames a wave's passes start at.
//
// One wave64 per utterance, several waves per workgroup, the passes of 64 frames of endpoint.hip and segment.hip (speech_frames.h's
// launch shape):
//   - the pass's 64 x C floats are copied coalesced into the wave's LDS slab with the odd lane stride C | 1; lane i then scans frame i's
//     classes in ascending order, three times at the most (maximum and label, the normaliser, the measure), and holds (label, q);
//   - a lane is the HEAD of a run when its label differs from its left neighbour's (lane 0 always is); a segmented inclusive scan over
//     the lanes (shuffles, six steps) gives every lane the minimum and the sum of q from its run's head up to itself -- at most 64 * 2^24
//     = 2^30, an int32;
//   - a lane whose right neighbour does not continue its run closes a token: its slot in tokens_out is the row's count so far plus the
//     number of closing lanes below it (a ballot and a prefix count).  The token that was open when the pass began lives in registers,
//     the same in every lane: a run that starts at lane 0 with its label continues it, and adds its 64-bit sum and minimum; otherwise
//     lane 0 closes it ahead of the pass's own tokens.  The last lane's run is carried on the same way;
//   - final closes what is open after the last pass; the slots past the row's count are filled with -1; the 16 state words are written
//     once, at the end.
// Every wave of a workgroup runs the same number of passes (those of the launch's `frames`), so the two barriers of a pass are uniform;
// lanes beyond a row's length load nothing -- the columns there may hold anything -- and take no part in any run.
#include "speech_frames.h"

namespace nbasr {
namespace {

constexpr int kStateWords = 16;
constexpr int kTokenWords = 8;                   // label, start, end, min_q, sum_lo, sum_hi, 0, 0
constexpr int kOne = 1 << 24;                    // q of confidence 1
constexpr int kNoLabel = -2;                     // a lane without a frame: no label equals it (-1 is the fresh prev_label)
enum { kProb = 0, kEntropy = 1, kTsallis = 2 };

__device__ inline void write_token(int* entry, int label, int start, int end, int min_q, long long sum)
{
    entry[0] = label; entry[1] = start; entry[2] = end; entry[3] = min_q;
    entry[4] = static_cast<int>(static_cast<unsigned long long>(sum) & 0xffffffffull);
    entry[5] = static_cast<int>(sum >> 32);
    entry[6] = 0; entry[7] = 0;
}

__device__ inline long long join64(int lo, int hi)
{
    return static_cast<long long>((static_cast<unsigned long long>(static_cast<unsigned>(hi)) << 32) | static_cast<unsigned>(lo));
}

// q of the frame at v[0 .. classes): steps 1 to 3 of the definition.  `forced`: the path's label (already in [0, classes)), or -1.
__device__ inline int quantised_confidence(const float* v, int classes, int forced, int measure, float alpha, float k, float ln_c, int* label)
{
    float m = v[0];
    int best = 0;
    for (int c = 1; c < classes; ++c) {
        const float val = v[c];
        if (val > m) { m = val; best = c; }                                 // the first maximum wins
    }
    const int at = forced >= 0 ? forced : best;
    *label = at;
    float s = 0.f;
    for (int c = 0; c < classes; ++c) s += expf(v[c] - m);
    const float lse = m + logf(s);
    float conf;
    if (measure == kProb) {
        conf = expf(v[at] - lse);
    } else if (measure == kEntropy) {
        float h = 0.f;
        for (int c = 0; c < classes; ++c) {
            const float lp = v[c] - lse, p = expf(lp);
            if (p != 0.f) h += p * lp;
        }
        conf = 1.f + h / ln_c;
    } else {
        float t = 0.f;
        for (int c = 0; c < classes; ++c) t += expf(alpha * (v[c] - lse));  // (exp(-inf) = 0: a masked class adds nothing)
        conf = (k - t) / (k - 1.f);
    }
    conf = fminf(fmaxf(conf, 0.f), 1.f);                                    // (fmaxf takes the number: a NaN becomes 0)
    return static_cast<int>(rintf(conf * 16777216.f));
}

__global__ __launch_bounds__(kSpeechMaxWaves * 64) void confidence_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const int* __restrict__ path, const int* state_in, int* state_out,
    int measure, float alpha, float k, float ln_c, int blank, int final_step, int* __restrict__ tokens_out,
    int* __restrict__ token_counts, int* __restrict__ q_out, int batch, int frames, int classes, int waves)
{
    extern __shared__ float lds_frames[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * waves + wave;
    const bool row = b < batch;                  // (a workgroup's last waves may have no row: they only keep the barriers)
    const int stride = classes | 1;
    float* slab = lds_frames + wave * 64 * stride;
    const size_t r = row ? b : 0;

    int g0 = 0, prev_label = -1, open_start = -1, open_min = kOne, count = 0, utt_min = kOne, utt_frames = 0, bad = 0;
    long long open_sum = 0, utt_sum = 0;
    int len = 0;
    if (row) {
        if (state_in) {
            const int* s = state_in + r * kStateWords;
            g0 = __builtin_amdgcn_readfirstlane(s[0]); prev_label = __builtin_amdgcn_readfirstlane(s[1]);
            open_start = __builtin_amdgcn_readfirstlane(s[2]); open_min = __builtin_amdgcn_readfirstlane(s[3]);
            open_sum = join64(__builtin_amdgcn_readfirstlane(s[4]), __builtin_amdgcn_readfirstlane(s[5]));
            count = __builtin_amdgcn_readfirstlane(s[6]); utt_min = __builtin_amdgcn_readfirstlane(s[7]);
            utt_sum = join64(__builtin_amdgcn_readfirstlane(s[8]), __builtin_amdgcn_readfirstlane(s[9]));
            utt_frames = __builtin_amdgcn_readfirstlane(s[10]); bad = __builtin_amdgcn_readfirstlane(s[11]);
        }
        len = __builtin_amdgcn_readfirstlane(lengths ? lengths[b] : frames);
        len = len < 0 ? 0 : (len > frames ? frames : len);                  // (lengths[b] <= frames is the caller's to keep: nothing beyond is read)
    }
    const float* xrow = x + r * frames * classes;
    int* tok = tokens_out ? tokens_out + r * (static_cast<size_t>(frames) + 1) * kTokenWords : nullptr;
    int closed = 0;                              // tokens this step has closed: the next free slot of tok

    for (int f0 = 0; f0 < frames; f0 += 64) {
        const int nf = len - f0 < 0 ? 0 : (len - f0 > 64 ? 64 : len - f0);  // this pass's frames of the row
        {                                                                   // the copy of speech_pass: element i = lane + 64 j is (frame f, class c)
            const float* src = xrow + static_cast<size_t>(f0) * classes;
            int f = lane / classes, c = lane - f * classes;
            const int df = 64 / classes, dc = 64 - df * classes;
            for (int i = lane; i < nf * classes; i += 64) {
                slab[f * stride + c] = src[i];
                f += df; c += dc;
                if (c >= classes) { c -= classes; ++f; }
            }
        }
        __syncthreads();

        const bool have = lane < nf;
        int label = kNoLabel, q = 0;
        bool bad_label = false;
        if (have) {
            int forced = -1;
            if (path) {
                forced = path[r * frames + f0 + lane];
                if (forced < 0 || forced >= classes) { forced = blank; bad_label = true; }
            }
            q = quantised_confidence(slab + lane * stride, classes, forced, measure, alpha, k, ln_c, &label);
        }
        if (row && q_out && f0 + lane < frames) q_out[r * frames + f0 + lane] = have ? q : -1;

        if (nf > 0) {                                                       // (wave-uniform)
            if (__ballot(bad_label) != 0ull) bad = 1;
            const bool token = have && label != blank;                      // a frame that belongs to a token
            const int left = __shfl_up(label, 1), right = __shfl_down(label, 1);
            const bool head = lane == 0 || !token || label != left;
            // the segmented inclusive scan: (mn, sm) of the frames from this lane's head up to this lane
            int mn = q, sm = q, seen = head ? 1 : 0;
            for (int d = 1; d < 64; d <<= 1) {
                const int mn_up = __shfl_up(mn, d), sm_up = __shfl_up(sm, d), seen_up = __shfl_up(seen, d);
                if (lane >= d && !seen) { mn = mn_up < mn ? mn_up : mn; sm += sm_up; seen = seen_up; }
            }
            const unsigned long long heads = __ballot(head);
            const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
            const int head_lane = 63 - __builtin_clzll(heads & upto);       // (bit 0 is always set)

            // the token that was open when the pass began: continued by the run at lane 0, or closed by lane 0
            const int label0 = __builtin_amdgcn_readfirstlane(label);
            const bool was_open = open_start >= 0;
            const bool continued = was_open && label0 == prev_label;
            const bool closes_carried = was_open && !continued;
            if (closes_carried) {
                if (tok && lane == 0) write_token(tok + static_cast<size_t>(closed) * kTokenWords, prev_label, open_start, g0, open_min, open_sum);
                ++closed;
            }
            const bool joins = continued && head_lane == 0;                 // this lane's run is the carried token's continuation
            const int run_start = joins ? open_start : g0 + head_lane;
            const int run_min = joins && open_min < mn ? open_min : mn;
            const long long run_sum = (joins ? open_sum : 0ll) + sm;

            // a token ends at this lane when the next frame of the pass does not continue it (the pass's last frame carries its run on)
            const bool ends = token && lane + 1 < nf && right != label;
            const unsigned long long enders = __ballot(ends);
            if (ends && tok) {
                const int slot = closed + __builtin_popcountll(enders & ((1ull << lane) - 1ull));
                write_token(tok + static_cast<size_t>(slot) * kTokenWords, label, run_start, g0 + lane + 1, run_min, run_sum);
            }
            closed += __builtin_popcountll(enders);

            // the utterance's own figures: every frame of a token
            int t_min = token ? q : kOne, t_sum = token ? q : 0;
            for (int d = 32; d > 0; d >>= 1) {
                const int other = __shfl_xor(t_min, d);
                t_min = other < t_min ? other : t_min;
                t_sum += __shfl_xor(t_sum, d);
            }
            utt_min = t_min < utt_min ? t_min : utt_min;
            utt_sum += t_sum;
            utt_frames += __builtin_popcountll(__ballot(token));

            // what the last frame of the pass leaves open
            const int last = nf - 1;
            const int last_label = __shfl(label, last);
            const int last_start = __shfl(run_start, last), last_min = __shfl(run_min, last);
            const int last_lo = __shfl(static_cast<int>(static_cast<unsigned long long>(run_sum) & 0xffffffffull), last);
            const int last_hi = __shfl(static_cast<int>(run_sum >> 32), last);
            prev_label = __builtin_amdgcn_readfirstlane(last_label);
            if (prev_label != blank) {
                open_start = __builtin_amdgcn_readfirstlane(last_start); open_min = __builtin_amdgcn_readfirstlane(last_min);
                open_sum = join64(__builtin_amdgcn_readfirstlane(last_lo), __builtin_amdgcn_readfirstlane(last_hi));
            } else {
                open_start = -1; open_min = kOne; open_sum = 0;
            }
            g0 += nf;
        }
        __syncthreads();                                                    // the slab is free for the next pass
    }

    if (final_step) {                                                       // the end of the row's frames closes what is open
        if (open_start >= 0) {
            if (row && tok && lane == 0) write_token(tok + static_cast<size_t>(closed) * kTokenWords, prev_label, open_start, g0, open_min, open_sum);
            ++closed;
        }
        prev_label = -1; open_start = -1; open_min = kOne; open_sum = 0;
    }
    if (!row) return;
    if (tok) {
        const int words = (frames + 1) * kTokenWords;
        for (int i = closed * kTokenWords + lane; i < words; i += 64) tok[i] = -1;
        if (lane == 0) token_counts[b] = closed;
    }
    if (lane < kStateWords) {
        const unsigned long long os = static_cast<unsigned long long>(open_sum), us = static_cast<unsigned long long>(utt_sum);
        const int words[kStateWords] = {g0, prev_label, open_start, open_min, static_cast<int>(os & 0xffffffffull), static_cast<int>(os >> 32),
                                        count + closed, utt_min, static_cast<int>(us & 0xffffffffull), static_cast<int>(us >> 32), utt_frames, bad,
                                        0, 0, 0, 0};
        int word = 0;
        for (int i = 0; i < kStateWords; ++i) word = lane == i ? words[i] : word;
        state_out[r * kStateWords + lane] = word;
    }
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_ctc_confidence_state_bytes(int batch)
{
    return batch <= 0 ? 0 : static_cast<size_t>(batch) * kStateWords * sizeof(int);
}

extern "C" int nbasr_ctc_confidence_step(const float* x, const int* lengths, const int* path, const int* state_in, int* state_out, int measure,
                                         float alpha, int blank, int final, int* tokens_out, int* token_counts, int* frame_q, int batch,
                                         int frames, int classes, nbasr_stream_t stream)
{
    static const char* who = "nbasr_ctc_confidence_step";
    clear_error();
    NBASR_REQUIRE(batch >= 0 && frames >= 0, NBASR_EINVAL, "%s: negative sizes (batch=%d, frames=%d)", who, batch, frames);
    NBASR_REQUIRE(classes >= 2 && classes <= kSpeechMaxClasses, NBASR_EINVAL, "%s: classes=%d must lie in [2, %d]", who, classes,
                  kSpeechMaxClasses);
    NBASR_REQUIRE(blank >= 0 && blank < classes, NBASR_EINVAL, "%s: blank=%d must lie in [0, %d)", who, blank, classes);
    NBASR_REQUIRE(measure >= kProb && measure <= kTsallis, NBASR_EINVAL, "%s: unknown measure %d (0 prob, 1 entropy, 2 tsallis)", who, measure);
    NBASR_REQUIRE(measure != kTsallis || (alpha > 0.f && alpha < 1.f), NBASR_EINVAL, "%s: alpha must lie strictly between 0 and 1 for tsallis",
                  who);                                                      // (refuses NaN too)
    NBASR_REQUIRE((tokens_out == nullptr) == (token_counts == nullptr), NBASR_EINVAL,
                  "%s: tokens_out and token_counts go together: give both or neither", who);
    NBASR_REQUIRE(state_out && (x || frames == 0 || batch == 0), NBASR_ENULL, "%s: NULL pointer (x and state_out are required)", who);
    if (batch == 0 || (frames == 0 && state_in == state_out && !final && !tokens_out)) return NBASR_OK;
    float k = 2.f;                                                          // (read by tsallis only)
    if (measure == kTsallis) k = static_cast<float>(std::pow(static_cast<double>(classes), 1.0 - static_cast<double>(alpha)));
    const float ln_c = static_cast<float>(std::log(static_cast<double>(classes)));
    const int slab_bytes = speech_slab_bytes(classes), waves = speech_waves(classes);
    const int blocks = (batch + waves - 1) / waves;
    hipLaunchKernelGGL(confidence_kernel, dim3(blocks), dim3(waves * 64), static_cast<size_t>(waves) * slab_bytes, as_stream(stream), x, lengths,
                       path, state_in, state_out, measure, alpha, k, ln_c, blank, final ? 1 : 0, tokens_out, token_counts, frame_q, batch,
                       frames, classes, waves);
    return launch_status(who);
}
