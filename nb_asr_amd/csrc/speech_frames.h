// The per-frame speech decision that endpoint.hip and segment.hip share (include/nbasr.h "endpointing", steps 1 and 2): a frame is
// SPEECH iff the largest value over the speech classes exceeds the largest over the others by more than `margin`.  One wave64 takes 64
// consecutive frames of its row, one lane per frame; the host side is the argument checks and the launch shape both steps use.
#pragma once
#include "common.h"

#include <cmath>

namespace nbasr {

constexpr int kSpeechMaxClasses = 128;
constexpr int kSpeechMaxWaves = 4;               // per workgroup
constexpr int kSpeechLdsBytes = 65536;           // a workgroup's slabs: waves * 64 * (C | 1) floats fit this

// One pass of a wave: is frame `lane` of the `nf` <= 64 frames at `src` (contiguous, `classes` floats each) speech?
//   - the pass's nf x C floats are contiguous in memory: the wave copies them coalesced into its LDS slab with an ODD lane stride (C | 1),
//     so the 32 lanes of a ds_read_b32 group land on 32 different banks while each lane scans its own frame in ascending class order;
//   - lanes at or beyond nf load nothing -- the columns there may hold anything -- and answer false.
// Holds one __syncthreads (after the copy): every wave of the workgroup calls it the same number of times, and the caller keeps a second
// barrier before the next call, when the slab is free again.
__device__ inline bool speech_pass(const float* __restrict__ src, float* slab, int nf, int classes, unsigned long long speech_lo,
                                   unsigned long long speech_hi, float margin, int lane)
{
    const int stride = classes | 1;
    int f = lane / classes, c = lane - f * classes;                         // element i = lane + 64 k of the pass is (frame f, class c)
    const int df = 64 / classes, dc = 64 - df * classes;
    for (int i = lane; i < nf * classes; i += 64) {
        slab[f * stride + c] = src[i];
        f += df; c += dc;
        if (c >= classes) { c -= classes; ++f; }
    }
    __syncthreads();

    bool speech = false;
    if (lane < nf) {
        const float* v = slab + lane * stride;
        float ms = -INFINITY, mn = -INFINITY;                               // maxima over the speech classes and over the others
        for (int k = 0; k < classes; ++k) {
            const bool in_s = ((k < 64 ? speech_lo >> k : speech_hi >> (k - 64)) & 1ull) != 0;
            const float val = v[k];
            if (in_s) { if (val > ms) ms = val; } else { if (val > mn) mn = val; }     // (a NaN is never taken)
        }
        speech = ms > mn + margin;
    }
    return speech;
}

// What both steps refuse about the frames and the speech set, in one wording; NBASR_OK when there is nothing to refuse.
inline int check_speech_args(const char* who, int batch, int frames, int classes, float margin, unsigned long long lo, unsigned long long hi)
{
    NBASR_REQUIRE(batch >= 0 && frames >= 0, NBASR_EINVAL, "%s: negative sizes (batch=%d, frames=%d)", who, batch, frames);
    NBASR_REQUIRE(classes >= 2 && classes <= kSpeechMaxClasses, NBASR_EINVAL, "%s: classes=%d must lie in [2, %d]", who, classes,
                  kSpeechMaxClasses);
    NBASR_REQUIRE(margin >= 0.f, NBASR_EINVAL, "%s: margin must be a number >= 0", who);                  // (refuses NaN too)
    const unsigned long long all_lo = classes >= 64 ? ~0ull : (1ull << classes) - 1ull;
    const unsigned long long all_hi = classes <= 64 ? 0ull : (classes == 128 ? ~0ull : (1ull << (classes - 64)) - 1ull);
    NBASR_REQUIRE((lo & ~all_lo) == 0 && (hi & ~all_hi) == 0, NBASR_EINVAL, "%s: the speech mask names classes at or above classes=%d", who,
                  classes);
    NBASR_REQUIRE(lo != 0 || hi != 0, NBASR_EINVAL, "%s: the speech set is empty", who);
    NBASR_REQUIRE(lo != all_lo || hi != all_hi, NBASR_EINVAL, "%s: the speech set is every class: no class is left for non-speech", who);
    return NBASR_OK;
}

inline int speech_slab_bytes(int classes) { return 64 * (classes | 1) * static_cast<int>(sizeof(float)); }

// Waves (= rows) per workgroup: as many slabs as fit the LDS budget, four at the most (128 classes: 33 KB a slab, one wave a workgroup).
inline int speech_waves(int classes)
{
    const int waves = kSpeechLdsBytes / speech_slab_bytes(classes);
    return waves > kSpeechMaxWaves ? kSpeechMaxWaves : waves;
}

}  // namespace nbasr
