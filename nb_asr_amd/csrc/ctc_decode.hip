// The reference's validation decode (reference training/torch/trainer.py:229-247 Trainer.decode):
//   CTCBeamDecoder(beam_width = 12, log_probs_input = True).decode(log_probs, output_len)   [ctcdecode, third-party C++]
//   -> PhonemeEncoder.fold_encoded(., 39)  -> torch_edit_distance.compute_wer(..., blank = [0], sep = [])  -> mean
// as two kernels: the CTC prefix beam search, and the label folding + blank removal + Levenshtein distance.
//
// Beam search (ctcdecode ctc_beam_search_decoder.cpp, no language model): per frame the vocabulary is cut to the
// `top_n` most probable classes; every live prefix keeps log P(ending in blank) and log P(ending in a non-blank); a prefix
// extended by class c is the SAME prefix as a live one that spells the same tokens (the trie of the C++ code), otherwise it
// is new; the `width` best of {live prefixes, new prefixes} by (score descending, last class ascending) survive.
//
// The frames of an utterance are a serial chain (250 at T = 1000), so the kernel is built for LATENCY: one wavefront per
// utterance, everything in registers.  Lane j holds live prefix j, lane c holds class c of the frame; values cross lanes by
// v_readlane (wave-uniform index) and DPP, not through LDS (a dependent LDS round trip costs ~130 cycles, an LDS atomic over
// the wavefront thousands).  Each lane tracks the best two candidates of its column (class); the survivors are picked by
// `width` rounds of a DPP wavefront maximum over 64-bit keys.  Prefix identity is a 64-bit hash of the token string (what
// the trie of ctcdecode provides; a re-created prefix must meet its still-live extensions again), the token strings
// themselves are (parent node, class) pairs in a per-utterance pool in global memory, walked backwards once at the end.
// All arithmetic is fp32 with ctcdecode's finite "-infinity" (-FLT_MAX).  The utterances of a batch run on different CUs.
//
// Per-token time steps (ctcdecode's fourth output; the TIMED instantiations, nbasr_ctc_beam_*_timed*): every token node carries a
// record (frame, best) after ctcdecode's PathTrie::get_path_trie -- the frame at which the node's class had the largest log-probability
// among the frames that extended into it.  A node is created with (t, lp_t[c]); at frame t a live prefix whose parent string is live
// too moves its own node's record to (t, lp_t[c]) when lp_t[c] is larger (strictly: the earliest frame wins).  The lane of a live
// prefix keeps `best` in a register, the frame lives in the pool: a timed node is two int2, (parent, class) then (frame, best).  The
// untimed instantiations compile to the code they were before the flag existed.
//
// Bigram fusion (ctcdecode's alpha / beta with a character scorer; the LM instantiations, nbasr_ctc_beam_*_lm*; the contract is in nbasr.h):
// one table W(classes, classes), W[p][c] added to the log score whenever a prefix ending in p is extended by c (row `blank`: the empty
// prefix).  W is staged once per launch into LDS, padded to 64 x 64.  The addresses a frame needs depend on the survivors of the previous
// frame only, so all of a frame's reads -- W[last_i][(lane + i) mod 64] for every live prefix i, and the one entry a live prefix's absorb
// rule needs -- are issued together at the top of the frame into an unrolled register array; the candidate scan (unrolled over BEAM_MAX for
// these instantiations, so the array is indexed by constants) adds them, and nothing in the rl / DPP chain waits on LDS.  A surviving
// extension takes its fused score back out of its key (the key transform is a bijection of the float's bits), which is the sum the scan
// formed, so materialising costs no dependent read either.  The instantiations without the flag compile to the code they were before.
#include "common.h"

#include <cfloat>
#include <climits>

namespace nbasr {

constexpr int BEAM_MAX = 32;                   // beam width limit (reference: 12)
constexpr int BEAM_CLASSES = 64;               // classes limit = lanes (reference: 49)
constexpr float NEG = -FLT_MAX;

__device__ __forceinline__ float log_sum_exp(float x, float y)
{
    if (x <= NEG) return y;
    if (y <= NEG) return x;
    const float m = fmaxf(x, y);
    return logf(expf(x - m) + expf(y - m)) + m;
}

// one add of a fusion table entry to a score that is not "-infinity"
__device__ __forceinline__ float beam_fuse(float v, float w) { return v > NEG ? v + w : v; }

// order-preserving key: larger = better.  score first, then the SMALLER last class (+1: the root's -1 becomes 0), then the
// smaller table slot (makes the choice between exact ties deterministic; ctcdecode leaves it to nth_element)
__device__ __forceinline__ unsigned long long beam_key(float score, int last_plus1, int slot)
{
    unsigned u = __float_as_uint(score);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return (static_cast<unsigned long long>(u) << 32) | (static_cast<unsigned long long>(0xFFFF - last_plus1) << 16) |
           static_cast<unsigned long long>(0xFFFF - slot);
}

// the score a key was made from, bit for bit (the transform of beam_key maps the floats one to one)
__device__ __forceinline__ float beam_key_score(unsigned long long key)
{
    const unsigned u = static_cast<unsigned>(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// Vocabulary pruning of ctcdecode (get_pruned_log_probs with cutoff_prob = 1): per frame only the top_n most probable classes
// take part (ties: lower class first).  Every frame is independent, so this runs as a wide pre-pass -- one wavefront per
// frame, lane = class -- instead of sitting in the serial frame chain of the search: pruned entries become -FLT_MAX.
__global__ __launch_bounds__(256) void ctc_prune_kernel(const float* __restrict__ log_probs, float* __restrict__ pruned,
                                                        long long n_frames, int classes, int top_n)
{
    const long long f = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= n_frames) return;
    const float lp = lane < classes ? log_probs[f * classes + lane] : NEG;
    int rank = 0;
    for (int c = 0; c < classes; ++c) {
        const float o = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(lp), c));      // c is wave-uniform
        rank += (o > lp || (o == lp && c < lane)) ? 1 : 0;
    }
    if (lane < classes) pruned[f * classes + lane] = rank < top_n ? lp : NEG;
}

__device__ __forceinline__ int rl(int v, int src) { return __builtin_amdgcn_readlane(v, src); }                 // src wave-uniform
__device__ __forceinline__ float rl(float v, int src) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), src)); }
__device__ __forceinline__ unsigned long long rl(unsigned long long v, int src)
{
    const unsigned lo = __builtin_amdgcn_readlane(static_cast<unsigned>(v), src), hi = __builtin_amdgcn_readlane(static_cast<unsigned>(v >> 32), src);
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src)
{
    const unsigned lo = __shfl(static_cast<unsigned>(v), src), hi = __shfl(static_cast<unsigned>(v >> 32), src);
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_max(unsigned long long v)
{
    const unsigned lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<unsigned>(v)), CTRL, 0xF, 0xF, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<unsigned>(v >> 32)), CTRL, 0xF, 0xF, false);
    const unsigned long long o = (static_cast<unsigned long long>(hi) << 32) | lo;
    return o > v ? o : v;
}

// maximum over the wavefront, wave-uniform result: butterfly inside each row of 16 lanes by DPP (quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, row_mirror), then the four rows by v_readlane
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
    v = dpp_max<0xB1>(v);
    v = dpp_max<0x4E>(v);
    v = dpp_max<0x141>(v);
    v = dpp_max<0x140>(v);
    const unsigned long long a = rl(v, 0), b = rl(v, 16), c = rl(v, 32), d = rl(v, 48);
    const unsigned long long ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

template <int CTRL>
__device__ __forceinline__ unsigned dpp_max(unsigned v)
{
    const unsigned o = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xF, 0xF, false));
    return o > v ? o : v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v)
{
    v = dpp_max<0xB1>(v);
    v = dpp_max<0x4E>(v);
    v = dpp_max<0x141>(v);
    v = dpp_max<0x140>(v);
    const unsigned a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const unsigned c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// the best 64-bit key of the wavefront (0: none).  The score occupies the high word, so a 32-bit maximum finds it; only when
// two lanes tie on the score exactly do the low words (last class, slot) have to be compared
__device__ __forceinline__ unsigned long long wave_best_key(unsigned long long mine)
{
    const unsigned hi = static_cast<unsigned>(mine >> 32);
    const unsigned top_hi = wave_max(hi);
    if (top_hi == 0u) return 0ull;
    const unsigned long long holders = __ballot(hi == top_hi);
    if (__popcll(holders) == 1) return rl(mine, __builtin_ctzll(holders));
    return wave_max(hi == top_hi ? mine : 0ull);
}

// rotate a value by one lane around the wavefront (DPP wave_rol:1)
__device__ __forceinline__ int wave_rotate(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x134, 0xF, 0xF, false); }
__device__ __forceinline__ float wave_rotate(float v) { return __int_as_float(wave_rotate(__float_as_int(v))); }

__device__ __forceinline__ unsigned long long extend_hash(unsigned long long h, int c)
{
    h = (h ^ static_cast<unsigned long long>(c + 1)) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

// The state of one utterance's search between two frames: lane j holds live prefix j (lanes >= n_live: unused, at the defaults
// of beam_lane_reset), lane c holds the merge mask of class c.  Pool nodes are (parent node, class) pairs; node 0 is the root.
struct BeamLanes {
    float p_b, p_nb, p_score;
    int p_last, p_node, p_len;
    int p_mp;                                       // index of the live prefix that is this one minus its last token, or -1
    unsigned long long p_hash, p_phash;
    unsigned merged;                                // class lane c: bit i set = (live prefix i + class c) is itself a live prefix
    int n_live, n_nodes;
    float p_best;                                   // TIMED only: `best` of this prefix's own node
};

__device__ __forceinline__ void beam_lane_reset(BeamLanes& s)
{
    s.p_b = s.p_nb = s.p_score = NEG; s.p_last = -1; s.p_node = 0; s.p_len = 0; s.p_mp = -1; s.p_hash = 0ull; s.p_phash = ~0ull;
    s.p_best = NEG;
}

// class lanes: the extensions that are live prefixes themselves (from p_mp and p_last of the live prefixes)
__device__ __forceinline__ unsigned merged_mask(int p_mp, int p_last, int n_live, int lane)
{
    unsigned merged = 0u;
    for (int j = 0; j < n_live; ++j) {
        const int mp = rl(p_mp, j), last = rl(p_last, j);
        if (mp >= 0 && lane == last) merged |= 1u << mp;
    }
    return merged;
}

// One frame of the prefix beam search: `lp` = log-probability of class `lane` in this frame (pruned: -FLT_MAX).  New prefixes get
// pool nodes n_nodes, n_nodes + 1, ... in rank order (at most `width` per frame).  The whole-utterance kernel and the resumable
// one both run exactly this, so the two cannot drift apart.  TIMED: `t` is the utterance's frame index, pool nodes are NODE_INT2<true> int2
// wide and carry their (frame, best) record; the owning lane writes a record when it creates a node or improves its own.
template <bool TIMED> constexpr int NODE_INT2 = TIMED ? 2 : 1;

// The fusion table of a launch in LDS, rows and columns padded to BEAM_CLASSES (the padding is never read: classes beyond `classes` are
// pruned, last classes are below `classes`); by all lanes of the workgroup.  Without LM: nothing, not a byte of LDS.
template <bool LM>
__device__ __forceinline__ const float* beam_stage_fusion(const float* __restrict__ fusion, int classes, int lane)
{
    if constexpr (LM) {
        __shared__ float s_w[BEAM_CLASSES * BEAM_CLASSES];
        // lane = column; 16 rows' loads are in flight before the first is stored (one load per trip costs a stream step of 10 frames
        // 10 us, as much as its frames' fusion)
        for (int p0 = 0; p0 < BEAM_CLASSES; p0 += 16) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = (p0 + k < classes && lane < classes) ? fusion[(p0 + k) * classes + lane] : 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s_w[(p0 + k) * BEAM_CLASSES + lane] = v[k];
        }
        __syncthreads();
        return s_w;
    } else {
        return nullptr;
    }
}

// X(0) X(1) ... X(BEAM_MAX - 1): the LM instantiations write their steps over the live prefixes out
#define BEAM_FOR_EACH_PREFIX(X)                                                                                                    \
    X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)                                          \
    X(16) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31)
static_assert(BEAM_MAX == 32, "BEAM_FOR_EACH_PREFIX lists BEAM_MAX steps");

// one step of the candidate scan: the extension of live prefix i by the class this lane holds after i rotations; W_ADD(v) fuses the table
#define BEAM_SCAN_STEP(W_ADD)                                                                                                      \
    {                                                                                                                              \
        const float sc = rl(p_score, i), bp = rl(p_b, i);                                                                          \
        const int last = rl(p_last, i);                                                                                            \
        const float v = W_ADD((cls == last) ? (bp > NEG ? lp_c + bp : NEG) : lp_c + sc);                                           \
        unsigned long long k = beam_key(v, cls + 1, i * BEAM_CLASSES + cls);                                                       \
        if (!(lp_c > NEG) || cls == blank || (((mrg | static_cast<int>(excluded)) >> i) & 1)) k = 0ull;                            \
        const unsigned long long lo = k < m1 ? k : m1;                                                                             \
        m1 = k > m1 ? k : m1;                                                                                                      \
        m2 = lo > m2 ? lo : m2;                                                                                                    \
        lp_c = wave_rotate(lp_c);                                                                                                  \
        cls = wave_rotate(cls);                                                                                                    \
        mrg = wave_rotate(mrg);                                                                                                    \
    }

// LM: `w_lds` = beam_stage_fusion's table; every score an extension contributes gets one add of W[the extended prefix's last class, or
// `blank` for the empty prefix][the class], after the acoustic sum is formed; a score of -FLT_MAX stays -FLT_MAX.
template <bool TIMED, bool LM>
__device__ __forceinline__ void beam_frame(BeamLanes& st, float lp, int2* __restrict__ pool, int classes, int width, int blank, int lane, int t,
                                           const float* __restrict__ w_lds)
{
    constexpr int NS = NODE_INT2<TIMED>;
    float p_b = st.p_b, p_nb = st.p_nb, p_score = st.p_score;
    int p_last = st.p_last, p_node = st.p_node, p_len = st.p_len, p_mp = st.p_mp;
    unsigned long long p_hash = st.p_hash, p_phash = st.p_phash;
    unsigned merged = st.merged;
    int n_live = st.n_live, n_nodes = st.n_nodes;
    const bool keep = lane < classes && lp > NEG;               // pruned by the pre-pass (or impossible): -FLT_MAX
    const float lpk = keep ? lp : NEG;
    const float lp_blank = rl(lpk, blank);

    // ---- live prefixes (lane j): stay on blank / repeat the last class / absorb the extension that spells the same tokens
    const float lp_last = __shfl(lpk, p_last >= 0 ? p_last : 0);
    const int par = p_mp >= 0 ? p_mp : 0;
    const float par_score = __shfl(p_score, par), par_b = __shfl(p_b, par);
    const int par_last = __shfl(p_last, par);
    // ---- LM: every table entry this frame can need, read now.  w_ext[i] = W[last of live prefix i][the class this lane holds at step i of
    //      the candidate scan, (lane + i) mod 64 (wave_rotate hands lane l the value of lane l + 1)]; w_abs = the entry of this lane's absorb
    //      rule, its parent's last class extended by its own.  Rows and columns are below BEAM_CLASSES by construction (a last class is -1
    //      or a class of a frame, `blank` < classes), so every read lies inside the staged tile.
    //      The steps over the live prefixes are written out BEAM_MAX times with one exit at the first i >= n_live: a loop with that exit
    //      is not unrolled, and a guard per step costs a taken branch for every step beyond n_live.
    float w_ext[LM ? BEAM_MAX : 1] = {};
    float w_abs = 0.f;
    if constexpr (LM) {
        w_abs = w_lds[(par_last >= 0 ? par_last : blank) * BEAM_CLASSES + (p_last >= 0 ? p_last : 0)];
#define BEAM_LOAD_STEP(i)                                                                                                          \
        if ((i) >= n_live) goto loaded;                                                                                            \
        {                                                                                                                          \
            const int last = rl(p_last, i);                                                                                        \
            w_ext[i] = w_lds[(last >= 0 ? last : blank) * BEAM_CLASSES + ((lane + (i)) & (BEAM_CLASSES - 1))];                     \
        }
        BEAM_FOR_EACH_PREFIX(BEAM_LOAD_STEP)
#undef BEAM_LOAD_STEP
    loaded:;
    }
    float n_b = NEG, n_nb = NEG, n_score = NEG;
    unsigned long long live_key = 0ull;
    if (lane < n_live) {
        n_b = lp_blank > NEG ? lp_blank + p_score : NEG;
        if (p_last >= 0 && lp_last > NEG) {
            n_nb = lp_last + p_nb;
            if (p_mp >= 0) {
                float add = p_last == par_last ? (par_b > NEG ? lp_last + par_b : NEG) : lp_last + par_score;
                if (LM && add > NEG) add += w_abs;
                n_nb = log_sum_exp(n_nb, add);
            }
        }
        n_score = log_sum_exp(n_b, n_nb);
        live_key = beam_key(n_score, p_last + 1, width * BEAM_CLASSES + lane);
    }
    // ---- TIMED: a live prefix whose parent string is live too was extended into by this frame (whether or not the parent can contribute
    //      probability, as ctcdecode's get_path_trie runs before log_p): a larger log-probability of its class moves its node's record here
    float p_best = TIMED ? st.p_best : 0.f;
    if (TIMED && lane < n_live && p_mp >= 0 && lp_last > NEG && lp_last > p_best) {
        p_best = lp_last;
        pool[p_node * NS + 1] = make_int2(t, __float_as_int(lp_last));
    }

    // The candidates (live prefix i + class c) are spread over the lanes by ROTATING the per-class values (log-probability,
    // class id, merge mask) one lane per live prefix: neither the extensions of one strong prefix nor those by one strong
    // class pile up in a single lane (a lane that wins more than twice in a frame has to rescan its candidates).
    // ---- candidates of column `lane`: the live prefix of this lane and the extensions of every live prefix by class `lane`;
    //      the best two are tracked, `taken` (bit i: extension of prefix i, bit 32: the live prefix) excludes picked ones
    unsigned long long taken = 0ull;
    auto column_scan = [=](unsigned long long excluded) -> ulonglong2 {
        unsigned long long m1 = (excluded >> 32) & 1ull ? 0ull : live_key, m2 = 0ull;
        float lp_c = lpk;                                        // log-probability of class (lane + i * step) mod 64
        int cls = lane, mrg = static_cast<int>(merged);
        if constexpr (LM) {                                      // unrolled: w_ext is indexed by constants and stays in registers
#define BEAM_FUSED(v) beam_fuse(v, w_ext[i])
#define BEAM_FUSED_STEP(I)                                                                                                         \
            if ((I) >= n_live) goto scanned;                                                                                       \
            {                                                                                                                      \
                constexpr int i = I;                                                                                               \
                BEAM_SCAN_STEP(BEAM_FUSED)                                                                                         \
            }
            BEAM_FOR_EACH_PREFIX(BEAM_FUSED_STEP)
#undef BEAM_FUSED_STEP
#undef BEAM_FUSED
        scanned:;
        } else {
#define BEAM_UNFUSED(v) v
            for (int i = 0; i < n_live; ++i) BEAM_SCAN_STEP(BEAM_UNFUSED)
#undef BEAM_UNFUSED
        }
        return make_ulonglong2(m1, m2);
    };
    ulonglong2 best = column_scan(0ull);
    unsigned long long mine = best.x, second = best.y;
    bool second_known = true;

    // ---- the `width` best of everything, best first: lane r keeps the winner of round r
    unsigned long long my_pick = 0ull;
    int n_next = 0;
    for (int r = 0; r < width; ++r) {
        const unsigned long long top = wave_best_key(mine);
        if (top == 0ull) break;                                    // fewer candidates than the beam is wide
        if (lane == r) my_pick = top;
        bool rescan = false;
        if (mine == top) {                                         // exactly one lane: the slot makes keys unique
            const int row = (0xFFFF - static_cast<int>(top & 0xFFFFu)) / BEAM_CLASSES;
            taken |= 1ull << (row == width ? 32 : row);
            if (second_known) { mine = second; second_known = false; }
            else rescan = true;
        }
        if (__any(rescan)) {                                       // by ALL lanes: the scan rotates values across the wavefront
            best = column_scan(taken);
            mine = best.x; second = best.y; second_known = true;
        }
        ++n_next;
    }

    // ---- the survivors become the live prefixes of the next frame: lane r gathers entry r from its source lane
    const int slot = 0xFFFF - static_cast<int>(my_pick & 0xFFFFu), row = slot / BEAM_CLASSES, col = slot % BEAM_CLASSES;
    const bool mine_valid = lane < n_next, survivor = row == width;
    const int src = mine_valid ? (survivor ? col : row) : 0;
    const float s_nb_new = __shfl(n_nb, src), s_b_new = __shfl(n_b, src), s_score_new = __shfl(n_score, src);
    const float s_b = __shfl(p_b, src), s_score = __shfl(p_score, src);
    const int s_last = __shfl(p_last, src), s_node = __shfl(p_node, src), s_len = __shfl(p_len, src);
    const unsigned long long s_hash = shfl64(p_hash, src), s_phash = shfl64(p_phash, src);
    const float s_best = TIMED ? __shfl(p_best, src) : 0.f;
    const float lp_col = __shfl(lpk, mine_valid && !survivor ? col : 0);
    if (mine_valid && survivor) {
        p_b = s_b_new; p_nb = s_nb_new; p_score = s_score_new;
        p_last = s_last; p_node = s_node; p_len = s_len; p_hash = s_hash; p_phash = s_phash;
        p_best = s_best;
    } else if (mine_valid) {
        // LM: the fused sum the scan formed for this candidate, as its key holds it (the same adds in the same order, without a table read)
        const float v = LM ? beam_key_score(my_pick) : (col == s_last) ? (s_b > NEG ? lp_col + s_b : NEG) : lp_col + s_score;
        p_b = NEG; p_nb = v; p_score = v;
        p_last = col; p_len = s_len + 1; p_phash = s_hash; p_hash = extend_hash(s_hash, col);
        p_node = -1 - s_node;                                       // parent's node, until this prefix gets its own
        p_best = lp_col;                                            // a new prefix, or a re-created one: a fresh record
    } else {
        p_b = p_nb = p_score = NEG; p_last = -1; p_node = 0; p_len = 0; p_hash = 0ull; p_phash = ~0ull;
        p_best = NEG;
    }
    // new pool nodes in rank order
    const bool is_new = mine_valid && p_node < 0;
    const unsigned long long new_mask = __ballot(is_new);
    if (is_new) {
        const int id = n_nodes + __popcll(new_mask & ((1ull << lane) - 1ull));
        pool[id * NS] = make_int2(-1 - p_node, p_last);
        if (TIMED) pool[id * NS + 1] = make_int2(t, __float_as_int(p_best));
        p_node = id;
    }
    n_nodes += __popcll(new_mask);
    n_live = n_next;
    // which live prefix is this one minus its last token (same length - 1, same token string)
    p_mp = -1;
    for (int i = 0; i < n_live; ++i)
        if (rl(p_hash, i) == p_phash && rl(p_len, i) + 1 == p_len) p_mp = i;
    if (lane >= n_live || p_last < 0) p_mp = -1;
    // class lanes: the extensions that are live prefixes themselves
    merged = merged_mask(p_mp, p_last, n_live, lane);
    st.p_b = p_b; st.p_nb = p_nb; st.p_score = p_score;
    st.p_last = p_last; st.p_node = p_node; st.p_len = p_len; st.p_mp = p_mp;
    st.p_hash = p_hash; st.p_phash = p_phash;
    st.merged = merged; st.n_live = n_live; st.n_nodes = n_nodes;
    if (TIMED) st.p_best = p_best;
}

// `len` frames of one utterance, rows of `classes` log-probabilities from lp_b on; frame t is the utterance's frame t0 + t (TIMED).
// The next frame's row is loaded before the current frame runs.  A macro, not a function: a helper is optimised on its own before it
// is inlined, and the frame body then lands 8 to 12 bytes earlier in the search and step kernels, which costs them 2 % (measured:
// profiles/streaming/beam_refactor_ab.json).  Expanded in place, the loop is compiled as it was when each kernel spelled it out.
#define BEAM_FRAMES(TIMED, LM, st, lp_b, len, pool, classes, width, blank, lane, t0, w_lds)                                        \
    do {                                                                                                                           \
        float lp_next = ((len) > 0 && (lane) < (classes)) ? (lp_b)[lane] : NEG;                                                    \
        for (int t = 0; t < (len); ++t) {                                                                                          \
            const float lp = lp_next;                                     /* class `lane` of frame t */                            \
            if (t + 1 < (len) && (lane) < (classes))                      /* in flight during this frame */                        \
                lp_next = (lp_b)[static_cast<size_t>(t + 1) * (classes) + (lane)];                                                 \
            beam_frame<TIMED, LM>(st, lp, pool, classes, width, blank, lane, (t0) + t, w_lds);                                     \
        }                                                                                                                          \
    } while (0)

// The rows of the search, the finish and the peek ("walk a beam's nodes backwards into its row, pad with 0") stay written out in their
// kernels.  One shared writer was measured: it moves the code around the frame loop of the search and the peek and costs the timed search
// 2.5 %, the timed peek 2 % and the width-1 search 3 % (profiles/streaming/beam_refactor_ab.json), for 15 lines saved.
// TIMED: timesteps(batch, width, frames) = the frame of every token's record, 0 beyond the beam's length.  (What the timed instantiations
// take in addition comes last in every kernel's arguments: the untimed ones read theirs where they always did.)
template <bool TIMED, bool LM>
__global__ __launch_bounds__(64) void ctc_beam_search_kernel(
    const float* __restrict__ log_probs, const int* __restrict__ lengths, int2* __restrict__ pool_all, int* __restrict__ beams,
    float* __restrict__ scores, int* __restrict__ beam_lens, int frames, int classes, int width, int blank, int* __restrict__ timesteps,
    const float* __restrict__ fusion)
{
    constexpr int NS = NODE_INT2<TIMED>;
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* w_lds = beam_stage_fusion<LM>(fusion, classes, lane);
    const int len = lengths ? min(max(lengths[b], 0), frames) : frames;
    int2* __restrict__ pool = pool_all + static_cast<size_t>(b) * (static_cast<size_t>(frames) * width + 1) * NS;
    const float* __restrict__ lp_b = log_probs + static_cast<size_t>(b) * frames * classes;

    // the empty prefix: P(blank-ending) = 1, hash 0, pool node 0
    BeamLanes st;
    beam_lane_reset(st);
    if (lane == 0) st.p_b = st.p_score = 0.f;
    st.merged = 0u;
    st.n_live = 1; st.n_nodes = 1;
    if (lane == 0) pool[0] = make_int2(-1, -1);

    BEAM_FRAMES(TIMED, LM, st, lp_b, len, pool, classes, width, blank, lane, 0, w_lds);

    // results, best first (the selection of the last frame already ordered them; a zero-length utterance has the empty prefix)
    __syncthreads();                                                   // pool entries written by other lanes
    if (lane < width) {
        int* out = beams + (static_cast<size_t>(b) * width + lane) * frames;
        int* out_t = TIMED ? timesteps + (static_cast<size_t>(b) * width + lane) * frames : nullptr;
        const bool live = lane < st.n_live;
        const int n = live ? st.p_len : 0;
        if (live) {
            int node = st.p_node;
            for (int k = n - 1; k >= 0; --k) {
                const int2 e = pool[node * NS];
                out[k] = e.y;
                if (TIMED) out_t[k] = pool[node * NS + 1].x;
                node = e.x;
            }
        }
        for (int k = n; k < frames; ++k) out[k] = 0;
        if (TIMED) for (int k = n; k < frames; ++k) out_t[k] = 0;
        scores[static_cast<size_t>(b) * width + lane] = live ? -st.p_score : FLT_MAX;     // ctcdecode returns -log P
        beam_lens[static_cast<size_t>(b) * width + lane] = n;
    }
}

// ---- resumable prefix beam search (streaming decode) ---------------------------------------------------------------------------
// The search of ctc_beam_search_kernel cut into chunks of frames, with the lanes' state stored between them.  Every candidate at
// frame t + 1 is a live prefix at frame t or a one-token extension of one, so the longest common TOKEN prefix of the live prefixes
// is a prefix of every beam the search can still return: after each chunk those tokens are committed (written out, never to change)
// and the pool is compacted -- the committed prefix becomes root node 0, only the nodes below it that a live lane reaches are kept,
// renumbered in their old order.  Hash and length keep covering the whole token string, so the search itself never sees the cut.
//
// State of one utterance, `beam_stream_record_bytes` bytes at a multiple of 8: a header of 16 ints (n_live, n_nodes, committed
// tokens, ended), then p_hash[width], p_phash[width] (u64), p_b, p_nb, p_score (f32) and p_last, p_node, p_len, p_mp (i32) per lane,
// then the pool (pool_nodes int2).  The pool comes last, so a larger pool keeps the layout of the smaller one's prefix.
// The timed state (nbasr_ctc_beam_stream_timed_*) is a layout of its own: the header also counts the utterance's frames so far, the
// lanes end with p_best (f32), and the pool's nodes are two int2 wide -- one wider node rather than a second array, so the pool is
// still the record's tail.
enum { BS_N_LIVE = 0, BS_N_NODES = 1, BS_COMMITTED = 2, BS_ENDED = 3, BS_FRAMES = 4, BS_HEADER_INTS = 16 };

__host__ __device__ constexpr size_t beam_stream_lanes_bytes(int width, bool timed = false)
{
    return (16 * static_cast<size_t>(width) + (timed ? 32 : 28) * static_cast<size_t>(width) + 7) & ~size_t(7);
}
__host__ __device__ constexpr size_t beam_stream_record_bytes(int width, int pool_nodes, bool timed = false)
{
    return BS_HEADER_INTS * 4 + beam_stream_lanes_bytes(width, timed) + static_cast<size_t>(pool_nodes) * (timed ? 2 : 1) * sizeof(int2);
}

struct BeamStreamRecord {
    int* hdr;
    unsigned long long *hash, *phash;
    float *pb, *pnb, *pscore;
    int *last, *node, *len, *mp;
    float* best;                                    // timed state only
    int2* pool;
};

__device__ __forceinline__ BeamStreamRecord beam_stream_record(char* state, int b, int width, int pool_nodes, bool timed = false)
{
    char* r = state + static_cast<size_t>(b) * beam_stream_record_bytes(width, pool_nodes, timed);
    BeamStreamRecord rec;
    rec.hdr = reinterpret_cast<int*>(r);
    rec.hash = reinterpret_cast<unsigned long long*>(r + BS_HEADER_INTS * 4);
    rec.phash = rec.hash + width;
    rec.pb = reinterpret_cast<float*>(rec.phash + width);
    rec.pnb = rec.pb + width;
    rec.pscore = rec.pnb + width;
    rec.last = reinterpret_cast<int*>(rec.pscore + width);
    rec.node = rec.last + width;
    rec.len = rec.node + width;
    rec.mp = rec.len + width;
    rec.best = reinterpret_cast<float*>(rec.mp + width);
    rec.pool = reinterpret_cast<int2*>(r + BS_HEADER_INTS * 4 + beam_stream_lanes_bytes(width, timed));
    return rec;
}

template <bool TIMED>
__device__ __forceinline__ void beam_stream_store(const BeamStreamRecord& rec, const BeamLanes& st, int lane, int width)
{
    if (lane < width) {
        rec.hash[lane] = st.p_hash; rec.phash[lane] = st.p_phash;
        rec.pb[lane] = st.p_b; rec.pnb[lane] = st.p_nb; rec.pscore[lane] = st.p_score;
        rec.last[lane] = st.p_last; rec.node[lane] = st.p_node; rec.len[lane] = st.p_len; rec.mp[lane] = st.p_mp;
        if (TIMED) rec.best[lane] = st.p_best;
    }
}

// The inverse of beam_stream_store: the lanes as the previous chunk left them (lanes >= n_live: the defaults the frame body gives them).
// n_live and n_nodes come from the record's header; the caller passes them, as it trusts them (the step) or clamped (the peek).
template <bool TIMED>
__device__ __forceinline__ BeamLanes beam_stream_load(const BeamStreamRecord& rec, int n_live, int n_nodes, int lane)
{
    BeamLanes st;
    beam_lane_reset(st);
    if (lane < n_live) {
        st.p_hash = rec.hash[lane]; st.p_phash = rec.phash[lane];
        st.p_b = rec.pb[lane]; st.p_nb = rec.pnb[lane]; st.p_score = rec.pscore[lane];
        st.p_last = rec.last[lane]; st.p_node = rec.node[lane]; st.p_len = rec.len[lane]; st.p_mp = rec.mp[lane];
        if (TIMED) st.p_best = rec.best[lane];
    }
    st.n_live = n_live; st.n_nodes = n_nodes;
    st.merged = merged_mask(st.p_mp, st.p_last, st.n_live, lane);
    return st;
}

template <bool TIMED>
__global__ __launch_bounds__(64) void ctc_beam_stream_init_kernel(char* __restrict__ state, int width, int pool_nodes)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const BeamStreamRecord rec = beam_stream_record(state, b, width, pool_nodes, TIMED);
    BeamLanes st;
    beam_lane_reset(st);
    if (lane == 0) st.p_b = st.p_score = 0.f;                         // the empty prefix: P(blank-ending) = 1, hash 0, node 0
    beam_stream_store<TIMED>(rec, st, lane, width);
    if (lane < BS_HEADER_INTS) rec.hdr[lane] = lane == BS_N_LIVE || lane == BS_N_NODES ? 1 : 0;
    if (lane == 0) rec.pool[0] = make_int2(-1, -1);
}

// lcp = the longest common token prefix of all n_live lanes beyond the `c_old` tokens committed before, in tokens (walked from the shortest
// suffix's depth upwards; once every lane stands on one node, the tokens above agree).  By all lanes, after the pool's writes are visible.
// A macro for BEAM_FRAMES' reason: as a function it moves the compaction loops behind it and the timed step loses 0.3 %.
#define BEAM_COMMON_PREFIX(lcp, st, pool, NS, c_old, lane)                                                                         \
    do {                                                                                                                           \
        const bool live_ = (lane) < (st).n_live;                                                                                   \
        int d_min = INT_MAX;                                                                                                       \
        for (int i = 0; i < (st).n_live; ++i) d_min = min(d_min, rl((st).p_len, i));                                               \
        d_min -= (c_old);                                             /* >= 0: every live prefix extends the committed one */      \
        int node = live_ ? (st).p_node : 0;                                                                                        \
        for (int skip = live_ ? (st).p_len - (c_old) - d_min : 0; skip > 0; --skip) node = (pool)[node * (NS)].x;                  \
        lcp = d_min;                                                                                                               \
        for (int k = d_min; k >= 1; --k) {                                                                                         \
            if (__ballot(live_ && node != rl(node, 0)) == 0ull) break;                                                             \
            const int2 e = live_ ? (pool)[node * (NS)] : make_int2(0, 0);                                                          \
            if (__ballot(live_ && e.y != rl(e.y, 0)) != 0ull) lcp = k - 1;                                                         \
            node = e.x;                                                                                                            \
        }                                                                                                                          \
    } while (0)

// One chunk of frames for every utterance (one wavefront each).  `ids`: pool_nodes ints of scratch per utterance (the renumbering).
// committed / partial: rows of pool_nodes ints (the host keeps usage + width * n + 1 <= pool_nodes, which bounds both counts).
// usage[b] = pool nodes in use afterwards, or -1: the chunk could overflow the pool, nothing was done.
// TIMED: committed_frames / partial_frames, rows like committed / partial, hold each written token's frame (counted per utterance from the
// init, over the frames of all steps that counted for it); the records move with their nodes through the compaction.
template <bool TIMED, bool LM>
__global__ __launch_bounds__(64) void ctc_beam_stream_kernel(
    const float* __restrict__ log_probs, const int* __restrict__ chunk_lengths, char* __restrict__ state, int* __restrict__ ids_all,
    int* __restrict__ committed, int* __restrict__ committed_counts, int* __restrict__ partial, int* __restrict__ partial_counts,
    int* __restrict__ usage, int frames, int classes, int width, int blank, int pool_nodes, int* __restrict__ committed_frames,
    int* __restrict__ partial_frames, const float* __restrict__ fusion)
{
    constexpr int NS = NODE_INT2<TIMED>;
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* w_lds = beam_stage_fusion<LM>(fusion, classes, lane);      // before the refusal below: a barrier every lane reaches
    const BeamStreamRecord rec = beam_stream_record(state, b, width, pool_nodes, TIMED);
    int2* __restrict__ pool = rec.pool;
    const int t0 = TIMED ? rec.hdr[BS_FRAMES] : 0;
    const int n_live0 = rec.hdr[BS_N_LIVE], n_nodes0 = rec.hdr[BS_N_NODES], c_old = rec.hdr[BS_COMMITTED], ended = rec.hdr[BS_ENDED];
    const int cl = chunk_lengths ? chunk_lengths[b] : frames;
    const int len = ended ? 0 : min(max(cl, 0), frames);
    if (static_cast<long long>(n_nodes0) + static_cast<long long>(width) * len + 1 > pool_nodes) {
        if (lane == 0) { usage[b] = -1; committed_counts[b] = 0; partial_counts[b] = 0; }
        return;
    }
    const float* __restrict__ lp_b = log_probs + static_cast<size_t>(b) * frames * classes;

    BeamLanes st = beam_stream_load<TIMED>(rec, n_live0, n_nodes0, lane);
    BEAM_FRAMES(TIMED, LM, st, lp_b, len, pool, classes, width, blank, lane, t0, w_lds);
    __syncthreads();                                                   // pool entries written by other lanes

    // ---- the committed prefix
    const int n_live = st.n_live;
    const bool live = lane < n_live;
    int lcp;
    BEAM_COMMON_PREFIX(lcp, st, pool, NS, c_old, lane);
    const int c_new = c_old + lcp;

    // ---- mark the nodes below the committed prefix that a live lane reaches; lane 0 (the best prefix) also writes its tokens:
    //      committed ones [c_old, c_new), then the partial suffix [c_new, p_len)
    int* __restrict__ ids = ids_all + static_cast<size_t>(b) * pool_nodes;
    const int n_nodes = st.n_nodes;
    for (int i = lane; i < n_nodes; i += 64) ids[i] = 0;
    __syncthreads();
    int* __restrict__ out_c = committed + static_cast<size_t>(b) * pool_nodes;
    int* __restrict__ out_p = partial + static_cast<size_t>(b) * pool_nodes;
    int* __restrict__ out_cf = TIMED ? committed_frames + static_cast<size_t>(b) * pool_nodes : nullptr;
    int* __restrict__ out_pf = TIMED ? partial_frames + static_cast<size_t>(b) * pool_nodes : nullptr;
    {
        const int stop = lane == 0 ? c_old : c_new;
        int k = live ? st.p_len : stop, nd = st.p_node;            // k: depth of node nd
        while (k > stop) {
            const int2 e = pool[nd * NS];
            if (k > c_new) ids[nd] = 1;
            if (lane == 0) {
                if (k > c_new) out_p[k - 1 - c_new] = e.y;
                else out_c[k - 1 - c_old] = e.y;
                if (TIMED) {
                    const int frame = pool[nd * NS + 1].x;
                    if (k > c_new) out_pf[k - 1 - c_new] = frame;
                    else out_cf[k - 1 - c_old] = frame;
                }
            }
            nd = e.x;
            --k;
        }
    }
    __syncthreads();
    // ---- new node ids in the old order (node 0 is never marked, so a marked node i gets an id <= i)
    int kept = 0;
    for (int i0 = 0; i0 < n_nodes; i0 += 64) {
        const int i = i0 + lane;
        const bool m = i < n_nodes && ids[i] != 0;
        const unsigned long long mask = __ballot(m);
        if (m) ids[i] = 1 + kept + __popcll(mask & ((1ull << lane) - 1ull));
        kept += __popcll(mask);
    }
    __syncthreads();
    // ---- move the kept nodes down, in place: a chunk of 64 reads its entries before it stores (the store data depends on them),
    //      and it stores only at ids <= its own indices.  The parent of a kept node is kept too, or it is the committed prefix (id 0).
    //      TIMED: the record half of a node moves the same way (its stores touch record halves only, and depend on its own loads).
    for (int i0 = 0; i0 < n_nodes; i0 += 64) {
        const int i = i0 + lane;
        const int id = i < n_nodes ? ids[i] : 0;
        int2 e = make_int2(0, 0), f = make_int2(0, 0);
        if (id) {
            e = pool[i * NS];
            e.x = ids[e.x];
            if (TIMED) f = pool[i * NS + 1];
        }
        if (id) pool[id * NS] = e;
        if (TIMED && id) pool[id * NS + 1] = f;
    }
    if (live) st.p_node = st.p_len > c_new ? ids[st.p_node] : 0;

    // ---- store the state
    beam_stream_store<TIMED>(rec, st, lane, width);
    if (lane == 0) {
        if (TIMED) rec.hdr[BS_FRAMES] = t0 + len;
        rec.hdr[BS_N_LIVE] = n_live;
        rec.hdr[BS_N_NODES] = 1 + kept;
        rec.hdr[BS_COMMITTED] = c_new;
        rec.hdr[BS_ENDED] = ended || (chunk_lengths && cl < frames) ? 1 : 0;
        usage[b] = 1 + kept;
        committed_counts[b] = lcp;
        partial_counts[b] = st.p_len - c_new;
    }
}

// The live prefixes' uncommitted suffixes, best first: beams(batch, width, ld) padded with 0, scores = -log P (FLT_MAX beyond
// n_live), beam_lens = suffix length (-1 beyond n_live).  Reads the state only.  TIMED: timesteps(batch, width, ld) = the suffix tokens' frames.
template <bool TIMED>
__global__ __launch_bounds__(64) void ctc_beam_stream_finish_kernel(const char* __restrict__ state, int* __restrict__ beams,
                                                                    float* __restrict__ scores, int* __restrict__ beam_lens, int ld,
                                                                    int width, int pool_nodes, int* __restrict__ timesteps)
{
    constexpr int NS = NODE_INT2<TIMED>;
    const int b = blockIdx.x, lane = threadIdx.x;
    const BeamStreamRecord rec = beam_stream_record(const_cast<char*>(state), b, width, pool_nodes, TIMED);
    if (lane >= width) return;
    const int n_live = rec.hdr[BS_N_LIVE], c = rec.hdr[BS_COMMITTED];
    const bool live = lane < n_live;
    const int n = live ? rec.len[lane] - c : 0;
    int* out = beams + (static_cast<size_t>(b) * width + lane) * ld;
    int* out_t = TIMED ? timesteps + (static_cast<size_t>(b) * width + lane) * ld : nullptr;
    if (live) {
        int node = rec.node[lane];
        for (int k = n - 1; k >= 0; --k) {
            const int2 e = rec.pool[node * NS];
            if (k < ld) out[k] = e.y;
            if (TIMED && k < ld) out_t[k] = rec.pool[node * NS + 1].x;
            node = e.x;
        }
    }
    for (int k = n; k < ld; ++k) out[k] = 0;
    if (TIMED) for (int k = n; k < ld; ++k) out_t[k] = 0;
    scores[static_cast<size_t>(b) * width + lane] = live ? -rec.pscore[lane] : FLT_MAX;
    beam_lens[static_cast<size_t>(b) * width + lane] = live ? n : -1;
}

// Nodes per utterance of a peek's scratch pool: the record's live nodes (at most pool_nodes) plus what `frames` frames can add.
__host__ __device__ constexpr size_t beam_stream_peek_nodes(int frames, int width, int pool_nodes)
{
    return static_cast<size_t>(pool_nodes) + static_cast<size_t>(width) * frames + 1;
}

// "Finish after these frames": what ctc_beam_stream_finish_kernel would write if ctc_beam_stream_kernel had first run on the chunk, with
// nothing committed, nothing compacted and no store to `state`.  The lanes are loaded from the record, the record's n_nodes live pool nodes
// are copied (at their indices, so the lanes' p_node stay valid) into a scratch pool of beam_stream_peek_nodes nodes, the shared frame body
// runs there, and the finish layout is written from the lanes in registers: suffixes after the record's committed prefix (the step would
// commit more of them, which moves tokens from the suffix to the head and changes no token).  The scratch holds the record's nodes and the
// chunk's, so there is no refusal for a full pool.  frames == 0 is the finish kernel.
template <bool TIMED, bool LM>
__global__ __launch_bounds__(64) void ctc_beam_stream_peek_kernel(
    const float* __restrict__ log_probs, const int* __restrict__ chunk_lengths, const char* __restrict__ state, int2* __restrict__ scratch_all,
    int* __restrict__ beams, float* __restrict__ scores, int* __restrict__ beam_lens, int ld, int frames, int classes, int width, int blank,
    int pool_nodes, int* __restrict__ timesteps, const float* __restrict__ fusion)
{
    constexpr int NS = NODE_INT2<TIMED>;
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* w_lds = beam_stage_fusion<LM>(fusion, classes, lane);
    const BeamStreamRecord rec = beam_stream_record(const_cast<char*>(state), b, width, pool_nodes, TIMED);
    const int2* __restrict__ src_pool = rec.pool;
    int2* __restrict__ pool = scratch_all + static_cast<size_t>(b) * beam_stream_peek_nodes(frames, width, pool_nodes) * NS;
    const int t0 = TIMED ? rec.hdr[BS_FRAMES] : 0;
    const int n_live0 = min(max(rec.hdr[BS_N_LIVE], 0), width), n_nodes0 = min(max(rec.hdr[BS_N_NODES], 1), pool_nodes);
    const int c_old = rec.hdr[BS_COMMITTED], ended = rec.hdr[BS_ENDED];
    const int cl = chunk_lengths ? chunk_lengths[b] : frames;
    const int len = ended ? 0 : min(max(cl, 0), frames);
    const float* __restrict__ lp_b = log_probs + static_cast<size_t>(b) * frames * classes;

    for (int i = lane; i < n_nodes0 * NS; i += 64) pool[i] = src_pool[i];
    __syncthreads();

    BeamLanes st = beam_stream_load<TIMED>(rec, n_live0, n_nodes0, lane);
    BEAM_FRAMES(TIMED, LM, st, lp_b, len, pool, classes, width, blank, lane, t0, w_lds);
    __syncthreads();                                                   // pool entries written by other lanes

    // TIMED: the step commits the longest common token prefix of the live prefixes and reports the committed tokens' frames from the BEST
    // prefix's nodes, for every beam.  Two live prefixes can spell that common part through different nodes with different records (a prefix
    // that left the beam and was created again has a fresh node), so the first `lcp` frames of every row are lane 0's here too.  The
    // tokens agree by definition, so the untimed peek needs none of this.
    const bool live = lane < st.n_live;
    int lcp = 0;
    if (TIMED) BEAM_COMMON_PREFIX(lcp, st, pool, NS, c_old, lane);                            // by all lanes

    if (lane >= width) return;
    const int n = live ? st.p_len - c_old : 0;
    int* out = beams + (static_cast<size_t>(b) * width + lane) * ld;
    int* out_t = TIMED ? timesteps + (static_cast<size_t>(b) * width + lane) * ld : nullptr;
    if (live) {
        int node = st.p_node;
        for (int k = n - 1; k >= 0; --k) {
            const int2 e = pool[node * NS];
            if (k < ld) out[k] = e.y;
            if (TIMED && k < ld) {
                const int frame = pool[node * NS + 1].x;
                if (k >= lcp) out_t[k] = frame;
                else if (lane == 0)
                    for (int r = 0; r < st.n_live; ++r) timesteps[(static_cast<size_t>(b) * width + r) * ld + k] = frame;
            }
            node = e.x;
        }
    }
    for (int k = max(n, 0); k < ld; ++k) out[k] = 0;
    if (TIMED) for (int k = max(n, 0); k < ld; ++k) out_t[k] = 0;
    scores[static_cast<size_t>(b) * width + lane] = live ? -st.p_score : FLT_MAX;
    beam_lens[static_cast<size_t>(b) * width + lane] = live ? n : -1;
}

// ---- label table + blank removal + Levenshtein distance, one workgroup per utterance -------------------------------------
// D[i][j] over anti-diagonals d = i + j: the cells of a diagonal are independent, three diagonals rotate through LDS
// (indexed by i).  Integer arithmetic: exact.
constexpr int EDIT_MAX = 2048;                 // tokens per sequence after blank removal

__global__ __launch_bounds__(256) void token_errors_kernel(
    const int* __restrict__ hyp, const int* __restrict__ hyp_len, int ld_hyp, const int* __restrict__ ref,
    const int* __restrict__ ref_len, int ld_ref, const int* __restrict__ table, int n_table, int blank, int* __restrict__ out)
{
    __shared__ int s_h[EDIT_MAX], s_r[EDIT_MAX];
    __shared__ int s_diag[3][EDIT_MAX + 1];
    __shared__ int s_count[2];
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { s_count[0] = s_count[1] = 0; s_bad = 0; }
    __syncthreads();
    // compaction in sequence order: wave 0 handles the hypothesis, wave 1 the reference (ballot prefix over 64-token chunks)
    if (tid < 128) {
        const int which = tid >> 6, lane = tid & 63;
        const int* src = which ? ref + static_cast<size_t>(b) * ld_ref : hyp + static_cast<size_t>(b) * ld_hyp;
        const int n = which ? min(max(ref_len[b], 0), ld_ref) : min(max(hyp_len[b], 0), ld_hyp);
        int* dst = which ? s_r : s_h;
        int count = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            int v = blank;
            if (i < n) {
                v = src[i];
                if (table) {
                    if (v < 0 || v >= n_table) { s_bad = 1; v = blank; }
                    else v = table[v];
                }
            }
            const bool keep = i < n && v != blank;
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
                if (pos < EDIT_MAX) dst[pos] = v;
            }
            count += __popcll(m);
        }
        if (lane == 0) s_count[which] = count;
    }
    __syncthreads();
    const int m = s_count[0], n = s_count[1];
    if (m > EDIT_MAX || n > EDIT_MAX || s_bad) {
        if (tid == 0) { out[2 * b] = -1; out[2 * b + 1] = s_bad ? -2 : -1; }
        return;
    }
    // diagonal d holds D[i][d - i] for max(0, d - n) <= i <= min(d, m)
    for (int d = 0; d <= m + n; ++d) {
        int* curd = s_diag[d % 3];
        const int* p1 = s_diag[(d + 2) % 3];      // d - 1
        const int* p2 = s_diag[(d + 1) % 3];      // d - 2
        const int lo = max(0, d - n), hi = min(d, m);
        for (int i = lo + tid; i <= hi; i += 256) {
            const int j = d - i;
            int v;
            if (i == 0) v = j;
            else if (j == 0) v = i;
            else {
                const int sub = p2[i - 1] + (s_h[i - 1] != s_r[j - 1] ? 1 : 0);
                v = min(min(p1[i - 1] + 1, p1[i] + 1), sub);        // D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + cost
            }
            curd[i] = v;
        }
        __syncthreads();
    }
    if (tid == 0) { out[2 * b] = s_diag[(m + n) % 3][m]; out[2 * b + 1] = n; }
}

}  // namespace nbasr

using namespace nbasr;

static size_t beam_pool_bytes(int batch, int frames, int beam_width, bool timed)
{
    return static_cast<size_t>(batch) * (static_cast<size_t>(frames) * beam_width + 1) * (timed ? 2 : 1) * sizeof(int2);
}

static size_t beam_workspace_bytes(int batch, int frames, int classes, int beam_width, bool timed)
{
    if (batch <= 0 || frames < 0 || classes <= 0 || beam_width <= 0) return 0;
    return beam_pool_bytes(batch, frames, beam_width, timed) + static_cast<size_t>(batch) * frames * classes * sizeof(float);
}

extern "C" size_t nbasr_ctc_beam_workspace_bytes(int batch, int frames, int classes, int beam_width)
{
    return beam_workspace_bytes(batch, frames, classes, beam_width, false);
}

extern "C" size_t nbasr_ctc_beam_timed_workspace_bytes(int batch, int frames, int classes, int beam_width)
{
    return beam_workspace_bytes(batch, frames, classes, beam_width, true);
}

// The prune pre-pass of a search over batch * frames rows, when the cutoff leaves classes out: `pruned` receives the rows the search
// should read.  -> the search's source (the log-probabilities themselves when nothing is cut)
static const float* beam_prune(const float* log_probs, float* pruned, int batch, int frames, int classes, int cutoff_top_n, hipStream_t s)
{
    if (cutoff_top_n >= classes || frames <= 0) return log_probs;
    const long long n_frames = static_cast<long long>(batch) * frames;
    hipLaunchKernelGGL(ctc_prune_kernel, dim3(static_cast<unsigned>((n_frames + 3) / 4)), dim3(256), 0, s, log_probs, pruned, n_frames,
                       classes, cutoff_top_n);
    return pruned;
}

// the untimed, the timed and the fused entry points share their checks; `timed` and `lm` select the kernel instantiation.  lm: `fusion` is
// the table (classes x classes floats on the device), refused when NULL before anything else is looked at
static int beam_search(const char* fn, bool timed, bool lm, const float* fusion, const float* log_probs, const int* lengths, void* ws, int* beams, float* scores,
                       int* timesteps, int* beam_lens, int batch, int frames, int classes, int beam_width, int blank, int cutoff_top_n,
                       nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && frames >= 0 && classes > 0 && blank >= 0 && blank < classes && cutoff_top_n > 0, NBASR_EINVAL,
                  "%s: bad sizes (batch=%d frames=%d classes=%d blank=%d cutoff_top_n=%d)", fn, batch, frames, classes, blank, cutoff_top_n);
    NBASR_REQUIRE(classes <= BEAM_CLASSES && beam_width >= 1 && beam_width <= BEAM_MAX, NBASR_EINVAL,
                  "%s: classes=%d (limit %d) / beam_width=%d (limit %d) unsupported", fn, classes, BEAM_CLASSES, beam_width, BEAM_MAX);
    NBASR_REQUIRE(!lm || fusion, NBASR_ENULL, "%s: NULL fusion table", fn);
    if (batch == 0) return NBASR_OK;
    NBASR_REQUIRE(ws && scores && beam_lens && (frames == 0 || (log_probs && beams && (!timed || timesteps))), NBASR_ENULL, "%s: NULL pointer", fn);
    NBASR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, NBASR_EALIGN, "%s: workspace must be 8-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    float* pruned = reinterpret_cast<float*>(static_cast<char*>(ws) + beam_pool_bytes(batch, frames, beam_width, timed));
    const float* src = beam_prune(log_probs, pruned, batch, frames, classes, cutoff_top_n, s);
    auto kernel = lm ? (timed ? ctc_beam_search_kernel<true, true> : ctc_beam_search_kernel<false, true>)
                     : (timed ? ctc_beam_search_kernel<true, false> : ctc_beam_search_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(64), 0, s, src, lengths, static_cast<int2*>(ws), beams, scores, beam_lens, frames, classes,
                       beam_width, blank, timesteps, fusion);
    return launch_status(fn);
}

extern "C" int nbasr_ctc_beam_search(const float* log_probs, const int* lengths, void* ws, int* beams, float* scores, int* beam_lens,
                                     int batch, int frames, int classes, int beam_width, int blank, int cutoff_top_n,
                                     nbasr_stream_t stream)
{
    return beam_search("nbasr_ctc_beam_search", false, false, nullptr, log_probs, lengths, ws, beams, scores, nullptr, beam_lens, batch, frames, classes,
                       beam_width, blank, cutoff_top_n, stream);
}

extern "C" int nbasr_ctc_beam_search_timed(const float* log_probs, const int* lengths, void* ws, int* beams, float* scores, int* timesteps,
                                           int* beam_lens, int batch, int frames, int classes, int beam_width, int blank, int cutoff_top_n,
                                           nbasr_stream_t stream)
{
    return beam_search("nbasr_ctc_beam_search_timed", true, false, nullptr, log_probs, lengths, ws, beams, scores, timesteps, beam_lens, batch,
                       frames, classes, beam_width, blank, cutoff_top_n, stream);
}

extern "C" int nbasr_ctc_beam_search_lm(const float* log_probs, const int* lengths, const float* fusion, void* ws, int* beams, float* scores,
                                        int* timesteps, int* beam_lens, int batch, int frames, int classes, int beam_width, int blank,
                                        int cutoff_top_n, int timed, nbasr_stream_t stream)
{
    return beam_search("nbasr_ctc_beam_search_lm", timed != 0, true, fusion, log_probs, lengths, ws, beams, scores, timed ? timesteps : nullptr,
                       beam_lens, batch, frames, classes, beam_width, blank, cutoff_top_n, stream);
}

static size_t beam_stream_state_bytes(int batch, int beam_width, int pool_nodes, bool timed)
{
    if (batch <= 0 || beam_width <= 0 || beam_width > BEAM_MAX || pool_nodes <= 0) return 0;
    return static_cast<size_t>(batch) * beam_stream_record_bytes(beam_width, pool_nodes, timed);
}

extern "C" size_t nbasr_ctc_beam_stream_state_bytes(int batch, int beam_width, int pool_nodes)
{
    return beam_stream_state_bytes(batch, beam_width, pool_nodes, false);
}

extern "C" size_t nbasr_ctc_beam_stream_timed_state_bytes(int batch, int beam_width, int pool_nodes)
{
    return beam_stream_state_bytes(batch, beam_width, pool_nodes, true);
}

extern "C" size_t nbasr_ctc_beam_stream_workspace_bytes(int batch, int frames, int classes, int pool_nodes)
{
    if (batch <= 0 || frames < 0 || classes <= 0 || pool_nodes <= 0) return 0;
    return static_cast<size_t>(batch) * pool_nodes * sizeof(int) + static_cast<size_t>(batch) * frames * classes * sizeof(float);
}

static int beam_stream_init(const char* fn, bool timed, void* state, int batch, int beam_width, int pool_nodes, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && pool_nodes >= 1, NBASR_EINVAL, "%s: bad sizes (batch=%d pool_nodes=%d)", fn, batch, pool_nodes);
    NBASR_REQUIRE(beam_width >= 1 && beam_width <= BEAM_MAX, NBASR_EINVAL, "%s: beam_width=%d (limit %d) unsupported", fn, beam_width, BEAM_MAX);
    if (batch == 0) return NBASR_OK;
    NBASR_REQUIRE(state, NBASR_ENULL, "%s: NULL pointer", fn);
    NBASR_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7u) == 0, NBASR_EALIGN, "%s: state must be 8-byte aligned", fn);
    auto kernel = timed ? ctc_beam_stream_init_kernel<true> : ctc_beam_stream_init_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(64), 0, as_stream(stream), static_cast<char*>(state), beam_width, pool_nodes);
    return launch_status(fn);
}

extern "C" int nbasr_ctc_beam_stream_init(void* state, int batch, int beam_width, int pool_nodes, nbasr_stream_t stream)
{
    return beam_stream_init("nbasr_ctc_beam_stream_init", false, state, batch, beam_width, pool_nodes, stream);
}

extern "C" int nbasr_ctc_beam_stream_timed_init(void* state, int batch, int beam_width, int pool_nodes, nbasr_stream_t stream)
{
    return beam_stream_init("nbasr_ctc_beam_stream_timed_init", true, state, batch, beam_width, pool_nodes, stream);
}

static int beam_stream_step(const char* fn, bool timed, bool lm, const float* fusion, const float* log_probs, const int* chunk_lengths, void* state, void* ws, int* committed,
                            int* committed_frames, int* committed_counts, int* partial, int* partial_frames, int* partial_counts, int* usage,
                            int batch, int frames, int classes, int beam_width, int blank, int cutoff_top_n, int pool_nodes, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && frames >= 0 && classes > 0 && blank >= 0 && blank < classes && cutoff_top_n > 0 && pool_nodes >= 1,
                  NBASR_EINVAL, "%s: bad sizes (batch=%d frames=%d classes=%d blank=%d cutoff_top_n=%d pool_nodes=%d)",
                  fn, batch, frames, classes, blank, cutoff_top_n, pool_nodes);
    NBASR_REQUIRE(classes <= BEAM_CLASSES && beam_width >= 1 && beam_width <= BEAM_MAX, NBASR_EINVAL,
                  "%s: classes=%d (limit %d) / beam_width=%d (limit %d) unsupported", fn, classes, BEAM_CLASSES, beam_width, BEAM_MAX);
    NBASR_REQUIRE(!lm || fusion, NBASR_ENULL, "%s: NULL fusion table", fn);
    if (batch == 0) return NBASR_OK;
    NBASR_REQUIRE(state && ws && committed && committed_counts && partial && partial_counts && usage && (frames == 0 || log_probs) &&
                      (!timed || (committed_frames && partial_frames)), NBASR_ENULL, "%s: NULL pointer", fn);
    NBASR_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7u) == 0, NBASR_EALIGN, "%s: state must be 8-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    float* pruned = reinterpret_cast<float*>(static_cast<char*>(ws) + static_cast<size_t>(batch) * pool_nodes * sizeof(int));
    const float* src = beam_prune(log_probs, pruned, batch, frames, classes, cutoff_top_n, s);
    auto kernel = lm ? (timed ? ctc_beam_stream_kernel<true, true> : ctc_beam_stream_kernel<false, true>)
                     : (timed ? ctc_beam_stream_kernel<true, false> : ctc_beam_stream_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(64), 0, s, src, chunk_lengths, static_cast<char*>(state), static_cast<int*>(ws), committed,
                       committed_counts, partial, partial_counts, usage, frames, classes, beam_width, blank, pool_nodes, committed_frames,
                       partial_frames, fusion);
    return launch_status(fn);
}

extern "C" int nbasr_ctc_beam_stream_step(const float* log_probs, const int* chunk_lengths, void* state, void* ws, int* committed,
                                          int* committed_counts, int* partial, int* partial_counts, int* usage, int batch, int frames,
                                          int classes, int beam_width, int blank, int cutoff_top_n, int pool_nodes, nbasr_stream_t stream)
{
    return beam_stream_step("nbasr_ctc_beam_stream_step", false, false, nullptr, log_probs, chunk_lengths, state, ws, committed, nullptr, committed_counts,
                            partial, nullptr, partial_counts, usage, batch, frames, classes, beam_width, blank, cutoff_top_n, pool_nodes, stream);
}

extern "C" int nbasr_ctc_beam_stream_timed_step(const float* log_probs, const int* chunk_lengths, void* state, void* ws, int* committed,
                                                int* committed_frames, int* committed_counts, int* partial, int* partial_frames,
                                                int* partial_counts, int* usage, int batch, int frames, int classes, int beam_width, int blank,
                                                int cutoff_top_n, int pool_nodes, nbasr_stream_t stream)
{
    return beam_stream_step("nbasr_ctc_beam_stream_timed_step", true, false, nullptr, log_probs, chunk_lengths, state, ws, committed,
                            committed_frames, committed_counts, partial, partial_frames, partial_counts, usage, batch, frames, classes, beam_width,
                            blank, cutoff_top_n, pool_nodes, stream);
}

extern "C" int nbasr_ctc_beam_stream_lm_step(const float* log_probs, const int* chunk_lengths, const float* fusion, void* state, void* ws,
                                             int* committed, int* committed_frames, int* committed_counts, int* partial, int* partial_frames,
                                             int* partial_counts, int* usage, int batch, int frames, int classes, int beam_width, int blank,
                                             int cutoff_top_n, int pool_nodes, int timed, nbasr_stream_t stream)
{
    return beam_stream_step("nbasr_ctc_beam_stream_lm_step", timed != 0, true, fusion, log_probs, chunk_lengths, state, ws, committed,
                            timed ? committed_frames : nullptr, committed_counts, partial, timed ? partial_frames : nullptr, partial_counts, usage,
                            batch, frames, classes, beam_width, blank, cutoff_top_n, pool_nodes, stream);
}

static int beam_stream_finish(const char* fn, bool timed, const void* state, int* beams, float* scores, int* timesteps, int* beam_lens,
                              int ld_beams, int batch, int beam_width, int pool_nodes, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && ld_beams >= 0 && pool_nodes >= 1, NBASR_EINVAL, "%s: bad sizes (batch=%d ld_beams=%d pool_nodes=%d)", fn, batch,
                  ld_beams, pool_nodes);
    NBASR_REQUIRE(beam_width >= 1 && beam_width <= BEAM_MAX, NBASR_EINVAL, "%s: beam_width=%d (limit %d) unsupported", fn, beam_width, BEAM_MAX);
    if (batch == 0) return NBASR_OK;
    NBASR_REQUIRE(state && scores && beam_lens && (ld_beams == 0 || (beams && (!timed || timesteps))), NBASR_ENULL, "%s: NULL pointer", fn);
    NBASR_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7u) == 0, NBASR_EALIGN, "%s: state must be 8-byte aligned", fn);
    auto kernel = timed ? ctc_beam_stream_finish_kernel<true> : ctc_beam_stream_finish_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(64), 0, as_stream(stream), static_cast<const char*>(state), beams, scores, beam_lens, ld_beams,
                       beam_width, pool_nodes, timesteps);
    return launch_status(fn);
}

extern "C" int nbasr_ctc_beam_stream_finish(const void* state, int* beams, float* scores, int* beam_lens, int ld_beams, int batch,
                                            int beam_width, int pool_nodes, nbasr_stream_t stream)
{
    return beam_stream_finish("nbasr_ctc_beam_stream_finish", false, state, beams, scores, nullptr, beam_lens, ld_beams, batch, beam_width,
                              pool_nodes, stream);
}

extern "C" int nbasr_ctc_beam_stream_timed_finish(const void* state, int* beams, float* scores, int* timesteps, int* beam_lens, int ld_beams,
                                                  int batch, int beam_width, int pool_nodes, nbasr_stream_t stream)
{
    return beam_stream_finish("nbasr_ctc_beam_stream_timed_finish", true, state, beams, scores, timesteps, beam_lens, ld_beams, batch,
                              beam_width, pool_nodes, stream);
}

// the peek's workspace: the scratch pools (8-byte nodes, or 16-byte ones for the timed family: sized for those, one size serves both), then
// the pruned log-probabilities
static size_t beam_stream_peek_pool_bytes(int batch, int frames, int beam_width, int pool_nodes)
{
    return static_cast<size_t>(batch) * beam_stream_peek_nodes(frames, beam_width, pool_nodes) * 2 * sizeof(int2);
}

extern "C" size_t nbasr_ctc_beam_stream_peek_workspace_bytes(int batch, int frames, int classes, int beam_width, int pool_nodes)
{
    if (batch <= 0 || frames < 0 || classes <= 0 || classes > BEAM_CLASSES || beam_width <= 0 || beam_width > BEAM_MAX || pool_nodes <= 0) return 0;
    const size_t pruned = (static_cast<size_t>(batch) * frames * classes * sizeof(float) + 7) & ~size_t(7);
    return beam_stream_peek_pool_bytes(batch, frames, beam_width, pool_nodes) + pruned;
}

static int beam_stream_peek(const char* fn, bool timed, bool lm, const float* fusion, const float* log_probs, const int* chunk_lengths, const void* state, void* ws, int* beams,
                            float* scores, int* timesteps, int* beam_lens, int ld_beams, int batch, int frames, int classes, int beam_width,
                            int blank, int cutoff_top_n, int pool_nodes, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && frames >= 0 && classes > 0 && blank >= 0 && blank < classes && cutoff_top_n > 0 && pool_nodes >= 1 && ld_beams >= 0,
                  NBASR_EINVAL, "%s: bad sizes (batch=%d frames=%d classes=%d blank=%d cutoff_top_n=%d pool_nodes=%d ld_beams=%d)",
                  fn, batch, frames, classes, blank, cutoff_top_n, pool_nodes, ld_beams);
    NBASR_REQUIRE(classes <= BEAM_CLASSES && beam_width >= 1 && beam_width <= BEAM_MAX, NBASR_EINVAL,
                  "%s: classes=%d (limit %d) / beam_width=%d (limit %d) unsupported", fn, classes, BEAM_CLASSES, beam_width, BEAM_MAX);
    NBASR_REQUIRE(!lm || fusion, NBASR_ENULL, "%s: NULL fusion table", fn);
    if (batch == 0) return NBASR_OK;
    NBASR_REQUIRE(state && ws && scores && beam_lens && (frames == 0 || log_probs) && (ld_beams == 0 || (beams && (!timed || timesteps))),
                  NBASR_ENULL, "%s: NULL pointer", fn);
    NBASR_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, NBASR_EALIGN,
                  "%s: state and workspace must be 8-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    float* pruned = reinterpret_cast<float*>(static_cast<char*>(ws) + beam_stream_peek_pool_bytes(batch, frames, beam_width, pool_nodes));
    const float* src = beam_prune(log_probs, pruned, batch, frames, classes, cutoff_top_n, s);
    auto kernel = lm ? (timed ? ctc_beam_stream_peek_kernel<true, true> : ctc_beam_stream_peek_kernel<false, true>)
                     : (timed ? ctc_beam_stream_peek_kernel<true, false> : ctc_beam_stream_peek_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(64), 0, s, src, chunk_lengths, static_cast<const char*>(state), static_cast<int2*>(ws), beams,
                       scores, beam_lens, ld_beams, frames, classes, beam_width, blank, pool_nodes, timesteps, fusion);
    return launch_status(fn);
}

extern "C" int nbasr_ctc_beam_stream_peek(const float* log_probs, const int* chunk_lengths, const void* state, void* ws, int* beams, float* scores,
                                          int* beam_lens, int ld_beams, int batch, int frames, int classes, int beam_width, int blank,
                                          int cutoff_top_n, int pool_nodes, nbasr_stream_t stream)
{
    return beam_stream_peek("nbasr_ctc_beam_stream_peek", false, false, nullptr, log_probs, chunk_lengths, state, ws, beams, scores, nullptr, beam_lens, ld_beams,
                            batch, frames, classes, beam_width, blank, cutoff_top_n, pool_nodes, stream);
}

extern "C" int nbasr_ctc_beam_stream_timed_peek(const float* log_probs, const int* chunk_lengths, const void* state, void* ws, int* beams,
                                                float* scores, int* timesteps, int* beam_lens, int ld_beams, int batch, int frames, int classes,
                                                int beam_width, int blank, int cutoff_top_n, int pool_nodes, nbasr_stream_t stream)
{
    return beam_stream_peek("nbasr_ctc_beam_stream_timed_peek", true, false, nullptr, log_probs, chunk_lengths, state, ws, beams, scores, timesteps,
                            beam_lens, ld_beams, batch, frames, classes, beam_width, blank, cutoff_top_n, pool_nodes, stream);
}

extern "C" int nbasr_ctc_beam_stream_lm_peek(const float* log_probs, const int* chunk_lengths, const float* fusion, const void* state, void* ws,
                                             int* beams, float* scores, int* timesteps, int* beam_lens, int ld_beams, int batch, int frames,
                                             int classes, int beam_width, int blank, int cutoff_top_n, int pool_nodes, int timed,
                                             nbasr_stream_t stream)
{
    return beam_stream_peek("nbasr_ctc_beam_stream_lm_peek", timed != 0, true, fusion, log_probs, chunk_lengths, state, ws, beams, scores,
                            timed ? timesteps : nullptr, beam_lens, ld_beams, batch, frames, classes, beam_width, blank, cutoff_top_n, pool_nodes,
                            stream);
}

extern "C" int nbasr_token_error_counts(const int* hyp, const int* hyp_len, int ld_hyp, const int* ref, const int* ref_len, int ld_ref,
                                        const int* table, int n_table, int blank, int* counts, int batch, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch >= 0 && ld_hyp >= 0 && ld_ref >= 0 && n_table >= 0, NBASR_EINVAL, "nbasr_token_error_counts: bad sizes");
    if (batch == 0) return NBASR_OK;
    NBASR_REQUIRE(hyp_len && ref_len && counts && (ld_hyp == 0 || hyp) && (ld_ref == 0 || ref) && (n_table == 0 || table), NBASR_ENULL,
                  "nbasr_token_error_counts: NULL pointer");
    hipLaunchKernelGGL(token_errors_kernel, dim3(batch), dim3(256), 0, as_stream(stream), hyp, hyp_len, ld_hyp, ref, ref_len, ld_ref,
                       n_table ? table : nullptr, n_table, blank, counts);
    return launch_status("nbasr_token_error_counts");
}
