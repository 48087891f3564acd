// What the two sample-tail streams share (internal; frontend_stream.hip and resample.hip, nb_asr_amd/frontend.py _SampleTailStream).
// A stream keeps the samples its next step still needs in one of two tails of tail_ld floats per utterance, used in turn: a step reads
// samples [tail_first, total_len) -- tail_len from tail_in, then n_new from wave -- and, unless it is final or tail_out is NULL, its
// trailing workgroup copies those from tail_first + tail_out_first_rel on into tail_out (that loop stays in each kernel: as a shared
// inline function it compiled to other instructions in both).  Both entry points check these arguments here, in three steps, because
// each checks what is its own between them and which refusal wins is part of the contract: tail_step_sizes; the step's early checks and
// "nothing to do"; tail_step_pointers; the step's checks of its outputs; tail_step_retain.
#pragma once
#include "common.h"

namespace nbasr {

inline int tail_step_sizes(const char* who, int tail_ld, int batch, int tail_len, long long tail_first, int n_new, int ld_wave, bool counts_ok,
                           long long total_len)      // counts_ok: the step's own counts (first output, outputs, col0) are not negative
{
    NBASR_REQUIRE(batch >= 0 && tail_len >= 0 && tail_len <= tail_ld && tail_first >= 0 && n_new >= 0 && ld_wave >= n_new && counts_ok,
                  NBASR_EINVAL, "%s: bad sizes", who);
    NBASR_REQUIRE(total_len == tail_first + tail_len + n_new, NBASR_EINVAL, "%s: total_len=%lld is not tail_first + tail_len + n_new = %lld", who,
                  total_len, tail_first + tail_len + n_new);
    return NBASR_OK;
}

inline int tail_step_pointers(const char* who, int batch, const float* tail_in, int tail_len, const float* wave, int n_new)
{
    NBASR_REQUIRE(batch <= 65535, NBASR_EINVAL, "%s: batch %d > 65535", who, batch);
    NBASR_REQUIRE((tail_in || tail_len == 0) && (wave || n_new == 0), NBASR_ENULL, "%s: NULL sample pointer", who);
    return NBASR_OK;
}

inline int tail_step_retain(const char* who, int tail_ld, const float* tail_in, int tail_len, int n_new, const float* tail_out,
                            int tail_out_first_rel)
{
    NBASR_REQUIRE(aligned16(tail_out), NBASR_EALIGN, "%s: tail_out must be 16-byte aligned", who);
    NBASR_REQUIRE(tail_out != tail_in, NBASR_EINVAL, "%s: tail_out must not be tail_in (two tails, used in turn)", who);
    NBASR_REQUIRE(tail_out_first_rel >= 0 && tail_out_first_rel <= tail_len + n_new && tail_len + n_new - tail_out_first_rel <= tail_ld,
                  NBASR_EINVAL, "%s: retaining %d samples, a tail holds %d", who, tail_len + n_new - tail_out_first_rel, tail_ld);
    return NBASR_OK;
}

namespace {

struct Samples {                                 // the stream's samples [tail_first, tail_first + tail_len + n_new) of one utterance
    const float* tail; const float* wave; long long tail_first; int tail_len; int n_new;
    __device__ __forceinline__ float at(long long i) const {
        const long long r = i - tail_first;
        if (r < 0) return 0.f;                   // (the host refuses a step that would need such a sample)
        if (r < tail_len) return tail[r];
        return r - tail_len < n_new ? wave[r - tail_len] : 0.f;
    }
};

}  // namespace
}  // namespace nbasr
