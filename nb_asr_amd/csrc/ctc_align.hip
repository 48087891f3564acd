// CTC forced alignment (nb_asr_amd.ctc forced_align; include/nbasr.h nbasr_ctc_forced_align): given the transcript, the best path
// through the blank-extended label sequence, the frames of every token and their scores.  The reference has no aligner; the definition
// is the one of include/nbasr.h, stated again in tests/ctc_align_model.py.  Where ctc_loss.hip sums over all paths, this kernel takes the
// maximum, keeps a 2-bit back-pointer per cell and walks them back.  One wavefront per utterance, as in ctc_loss.hip.
#include "common.h"

namespace nbasr {
namespace {

constexpr int ALIGN_MAX_LABELS = 1024;
constexpr int ALIGN_MAX_POS = 2 * ALIGN_MAX_LABELS + 1;
constexpr int WALK_ROWS = 16;                  // back-pointer rows fetched per batch of the walk (one batch is in flight ahead of the walk)

// A single wavefront needs no barrier: its LDS operations execute in issue order; this only keeps the compiler from reordering them.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane i owns the positions i, i + 64, ...  The kernel is compiled for every count of GROUPS of four positions per lane (256 positions
// of the label sequence) that ld_targets can ask for, so that the sweep over a frame has no branch in it; a lane's 2-bit back-pointers are
// packed 16 to a 32-bit word, NW = ceil(GROUPS / 4) words per lane and frame.
inline int align_groups(int ld_targets) { return (2 * ld_targets + 1 + 255) / 256; }
inline int align_words(int ld_targets) { return (align_groups(ld_targets) + 3) / 4; }

// Back-pointer workspace: word w of lane i in frame t of utterance b sits at ((b * frames + t) * NW + w) * 64 + i, so a frame's row is NW
// coalesced stores of 64 words.  Word w holds the positions i + 64 (16 w + kk), kk = 0..15, i.e. [1024 w, 1024 w + 1023]; bits 2kk, 2kk+1 =
// how far the best predecessor lies below (0 stay, 1, 2).  Frame 0 has no predecessor: its row is never written or read.  Every lane
// reads back only the words it wrote itself, so the workspace needs no ordering between lanes.
template <int GROUPS>
__global__ __launch_bounds__(64) void ctc_align_kernel(const float* __restrict__ log_probs, const int* __restrict__ lengths,
                                                       const int* __restrict__ targets, const int* __restrict__ target_lengths,
                                                       uint32_t* __restrict__ ws, float* __restrict__ scores, int* __restrict__ path,
                                                       int* __restrict__ starts, int* __restrict__ ends, float* __restrict__ token_scores,
                                                       int frames, int classes, int ld_targets, int blank)
{
    constexpr int PPL = 4 * GROUPS;                                     // positions per lane the sweep computes (those beyond the last one are idle)
    constexpr int NW = (GROUPS + 3) / 4;
    __shared__ float s_v[2][2 + ALIGN_MAX_POS + 1];             // v(s) at [2 + s]: two cells of -inf below s = 0, a spare cell for the idle positions above
    __shared__ int s_label[ALIGN_MAX_POS];
    __shared__ int s_start[ALIGN_MAX_LABELS], s_end[ALIGN_MAX_LABELS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int len = min(max(lengths[b], 0), frames);
    const int n_lab = min(max(target_lengths[b], 0), ld_targets);
    const int n_pos = 2 * n_lab + 1;
    const float ninf = -INFINITY;
    const float* __restrict__ lp_b = log_probs + static_cast<size_t>(b) * frames * classes;
    uint32_t* __restrict__ ws_b = ws + static_cast<size_t>(b) * frames * (NW * 64);
    int* __restrict__ path_b = path + static_cast<size_t>(b) * frames;
    bool bad = false;
    for (int s = lane; s < n_pos; s += 64) {
        int lab = blank;
        if (s & 1) {
            lab = targets[static_cast<size_t>(b) * ld_targets + (s >> 1)];
            if (lab < 0 || lab >= classes || lab == blank) { bad = true; lab = blank; }
        }
        s_label[s] = lab;
    }
    for (int j = lane; j < n_lab; j += 64) s_start[j] = s_end[j] = -1;
    wave_sync();
    const bool any_bad = __any(bad);

    // ---- forward sweep: v_t(s) = max over the allowed predecessors + lp[t][l'_s]; ties go to the smallest step ------------------------
    float score = ninf;
    int s_last = 0;
    if (!any_bad && len > 0) {
        // This lane's labels and whether s - 2 may precede s are fixed over the frames.  Nothing in a frame's sweep branches: v has two cells of
        // -inf below s = 0, positions beyond the last one read the last one and write to a spare cell, so the LDS reads of a frame are issued
        // back to back.  The log-probabilities a lane needs, lp[t][l'_s], are fetched one frame ahead of their use.
        int lab[PPL];
        bool skip[PPL];
        float lp_next[PPL];
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
            const int s = lane + 64 * k;
            lab[k] = s < n_pos ? s_label[s] : blank;
            skip[k] = s > 1 && s < n_pos && lab[k] != blank && lab[k] != s_label[s - 2];
            lp_next[k] = lp_b[static_cast<size_t>(min(1, len - 1)) * classes + lab[k]];
        }
        // t = 0: only the first blank and the first label are reachable
        if (lane < 2) s_v[0][lane] = s_v[1][lane] = ninf;
        for (int s = lane; s < n_pos; s += 64) s_v[0][2 + s] = s < 2 ? lp_b[s_label[s]] : ninf;
        wave_sync();
        int cur = 0;
        for (int t = 1; t < len; ++t) {
            const float* prev = s_v[cur] + 2;
            float* next = s_v[cur ^ 1] + 2;
            const float* __restrict__ row = lp_b + static_cast<size_t>(min(t + 1, len - 1)) * classes;
            uint32_t* __restrict__ wrow = ws_b + static_cast<size_t>(t) * (NW * 64);
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                uint32_t bits = 0;
#pragma unroll
                for (int k = 16 * w; k < 16 * w + 16 && k < PPL; ++k) {
                    const int s = lane + 64 * k, sc = min(s, n_pos - 1);
                    const float a1 = prev[sc - 1];
                    const float a2 = skip[k] ? prev[sc - 2] : ninf;
                    float m = prev[sc];
                    uint32_t step = 0;
                    if (a1 > m) { m = a1; step = 1; }
                    if (a2 > m) { m = a2; step = 2; }
                    next[s < n_pos ? s : ALIGN_MAX_POS] = m + lp_next[k];
                    bits |= (s < n_pos ? step : 0u) << (2 * (k & 15));
                    lp_next[k] = row[lab[k]];                            // its value is spent: the load lands in the register itself
                }
                wrow[64 * w + lane] = bits;
            }
            cur ^= 1;
            wave_sync();
        }
        // the path ends on the last label or on the last blank; on a tie on the label
        const float l1 = s_v[cur][2 + n_pos - 1], l2 = n_pos > 1 ? s_v[cur][2 + n_pos - 2] : ninf;
        const bool on_label = n_pos > 1 && l2 >= l1;
        score = on_label ? l2 : l1;
        s_last = on_label ? n_pos - 2 : n_pos - 1;
    } else if (!any_bad && n_lab == 0) {
        score = 0.f;                                                     // nothing to emit in no frames
    }
    if (lane == 0) scores[b] = any_bad ? NAN : score;
    const bool walk = !any_bad && len > 0 && score != ninf;             // -inf: no path (too few frames, or every path crosses a masked class)
    for (int t = (walk ? len : 0) + lane; t < frames; t += 64) path_b[t] = -1;

    // ---- backtrack ------------------------------------------------------------------------------------------------------------------------
    // Which rows the walk needs does not depend on the path, only which lane's word and which bit pair: every lane fetches its own words
    // of WALK_ROWS rows at a time, one batch ahead of the walk, and the walk takes the owner's word with a cross-lane read (v_readlane; the
    // position is wave-uniform).  Lane j of a chunk of 64 frames keeps the position of frame top - j; the chunk's path goes out as one store,
    // and a lane that sees its neighbour frame at another position knows a token's first or last frame.
    if (walk) {
        int s_cur = __builtin_amdgcn_readfirstlane(s_last);
        int s_above = -1;                                                // position of the frame above the current chunk (none above the last frame)
        int my_s = -1;
        const int batches = (len + WALK_ROWS - 1) / WALK_ROWS;
        uint32_t rows[WALK_ROWS][NW], rows_next[WALK_ROWS][NW];
        auto fetch = [&](uint32_t (&dst)[WALK_ROWS][NW], int top) {
#pragma unroll
            for (int r = 0; r < WALK_ROWS; ++r)
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const int t = top - r;
                    dst[r][w] = t >= 1 ? ws_b[static_cast<size_t>(t) * (NW * 64) + 64 * w + lane] : 0u;
                }
        };
        fetch(rows, len - 1);
        for (int q = 0; q < batches; ++q) {
            const int top = len - 1 - WALK_ROWS * q;
            if (q + 1 < batches) fetch(rows_next, top - WALK_ROWS);
#pragma unroll
            for (int r = 0; r < WALK_ROWS; ++r) {
                const int t = top - r;
                if (t >= 0) {
                    if (lane == ((WALK_ROWS * q + r) & 63)) my_s = s_cur;
                    if (t >= 1) {
                        const int k = s_cur >> 6;
                        uint32_t word = rows[r][0];
#pragma unroll
                        for (int w = 1; w < NW; ++w) if ((k >> 4) == w) word = rows[r][w];
                        const uint32_t owners = __builtin_amdgcn_readlane(word, s_cur & 63);
                        s_cur = __builtin_amdgcn_readfirstlane(s_cur - static_cast<int>((owners >> (2 * (k & 15))) & 3u));
                    }
                }
            }
            if ((q & 3) == 3 || q == batches - 1) {                    // a chunk of 64 frames is complete (or the walk is)
                const int t = len - 1 - 64 * (q >> 2) - lane;
                const int up = __shfl_up(my_s, 1), down = __shfl_down(my_s, 1);
                if (t >= 0) {
                    const int above = lane == 0 ? s_above : up;
                    const int below = t == 0 ? -1 : (lane == 63 ? s_cur : down);
                    path_b[t] = s_label[my_s];
                    if (my_s & 1) {
                        if (above != my_s) s_end[my_s >> 1] = t + 1;
                        if (below != my_s) s_start[my_s >> 1] = t;
                    }
                }
                s_above = __builtin_amdgcn_readlane(my_s, 63);
            }
            if (q + 1 < batches) {
#pragma unroll
                for (int r = 0; r < WALK_ROWS; ++r)
#pragma unroll
                    for (int w = 0; w < NW; ++w) rows[r][w] = rows_next[r][w];
            }
        }
    }
    wave_sync();

    // ---- spans and token scores: lanes over tokens, each token's frames added in increasing order --------------------------------------------
    for (int j = lane; j < ld_targets; j += 64) {
        int first = -1, last = -1;
        float sum = 0.f;
        if (walk && j < n_lab) {
            first = s_start[j];
            last = s_end[j];
            const int lab = s_label[2 * j + 1];
            if (first >= 0)
#pragma unroll 4
                for (int t = first; t < last; ++t) sum += lp_b[static_cast<size_t>(t) * classes + lab];
        }
        const size_t at = static_cast<size_t>(b) * ld_targets + j;
        starts[at] = first;
        ends[at] = last;
        token_scores[at] = sum;
    }
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_ctc_align_workspace_bytes(int batch, int frames, int ld_targets)
{
    if (batch <= 0 || frames <= 0 || ld_targets < 0 || ld_targets > ALIGN_MAX_LABELS) return 0;
    return static_cast<size_t>(batch) * frames * align_words(ld_targets) * 64 * sizeof(uint32_t);
}

extern "C" int nbasr_ctc_forced_align(const float* log_probs, const int* lengths, const int* targets, const int* target_lengths, void* ws,
                                      float* scores, int* path, int* starts, int* ends, float* token_scores, int batch, int frames, int classes,
                                      int ld_targets, int blank, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && frames >= 0 && classes > 0 && ld_targets >= 0 && blank >= 0 && blank < classes, NBASR_EINVAL,
                  "nbasr_ctc_forced_align: bad sizes (batch=%d frames=%d classes=%d ld_targets=%d blank=%d)", batch, frames, classes, ld_targets, blank);
    NBASR_REQUIRE(ld_targets <= ALIGN_MAX_LABELS, NBASR_EINVAL, "nbasr_ctc_forced_align: at most %d labels per utterance, got ld_targets=%d",
                  ALIGN_MAX_LABELS, ld_targets);
    if (batch == 0) return NBASR_OK;
    NBASR_REQUIRE(lengths && target_lengths && scores && (frames == 0 || (log_probs && ws && path)) &&
                      (ld_targets == 0 || (targets && starts && ends && token_scores)),
                  NBASR_ENULL, "nbasr_ctc_forced_align: NULL pointer");
    static constexpr decltype(&ctc_align_kernel<1>) kernels[9] = {ctc_align_kernel<1>, ctc_align_kernel<2>, ctc_align_kernel<3>, ctc_align_kernel<4>, ctc_align_kernel<5>,
                                                                  ctc_align_kernel<6>, ctc_align_kernel<7>, ctc_align_kernel<8>, ctc_align_kernel<9>};
    hipLaunchKernelGGL(kernels[align_groups(ld_targets) - 1], dim3(batch), dim3(64), 0, as_stream(stream), log_probs, lengths, targets, target_lengths,
                       static_cast<uint32_t*>(ws), scores, path, starts, ends, token_scores, frames, classes, ld_targets, blank);
    return launch_status("nbasr_ctc_forced_align");
}
