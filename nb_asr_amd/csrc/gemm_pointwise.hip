// Per-frame linear maps  y[b][co][t] = sum_ci W[co][ci] x[b][ci][t] + bias  on the matrix cores, ONE kernel template for two operand
// schemes (as gemm_conv_split.hip is for the k = 8 convolution):
//   * the `linear` node op of a search cell (reference ops.py:42-50: permute, Linear, ReLU, min(20), permute) + the node's
//     skip sum (model.py:13-22);
//   * the LSTM input projection (model.py:100,118-121), stored time-major.
//
//   PwF16x2  fp32 rows, fp32-accurate through the two-way operand split of gemm_conv_split.hip (v = hi + lo' 2^-11, three
//            v_mfma_f32_16x16x32_f16 per product); both operands range-normalised by powers of two.
//   PwBf16   the bf16 storage path (BASELINE config 4: model.to(torch.bfloat16)): every tensor of the bf16 model IS a bfloat16 tensor and
//            so is every weight, so the products go to v_mfma_f32_16x16x32_bf16 unchanged, ONE MFMA per product: exact bf16 x bf16
//            products, fp32 accumulation -- the reference's arithmetic up to the order of the sums; the normalised input is rounded to
//            bf16 exactly where the reference's LayerNorm module rounds its output.  No scales: bf16 has fp32's exponent range.
//
// Unlike the k=8 convolution a pointwise map re-uses nothing along the frame axis, so splitting x inside the GEMM would cost
// as much vector work as the MFMAs it feeds (and every row tile would repeat it).  The activation is therefore converted ONCE
// by a streaming pre-pass into the exact LDS image the GEMM wants, and the GEMM moves BOTH operands with LDS-DMA only:
//
//   image:  x (batch, C, ld) fp32 / bf16 [+ pending LayerNorm]  ->  image[b][frame tile of 256][K-step of 32 channels]
//             PwF16x2  [split][16-channel block][8-channel half][256 frames][8 channels] fp16   (32 KiB per (tile, K-step), contiguous)
//                      with ONE power-of-two scale per (utterance, frame tile): a pointwise map never mixes frames, so the scale
//                      can be that local; the largest magnitude of the tile lands in [2^14, 2^15);
//             PwBf16          [16-channel block][8-channel half][256 frames][8 channels] bf16   (16 KiB per (tile, K-step), contiguous)
//   weights: (c_out, c_in) fp32  ->  [row tile of 128][K-step]
//             PwF16x2  [split][block][half][128 rows][8 ch] fp16 (16 KiB), then per-row 2^kw and 2^-kw;
//             PwBf16          [block][half][128 rows][8 ch] bf16 (8 KiB) -- the values of a bf16 parameter: the rounding is exact;
//   GEMM:   128 x 256 tile per 512-thread workgroup (8 waves of 64 x 64 = 4 x 4 MFMA tiles), K-step = 32 channels = one MFMA k-block;
//           per step the packed weights + the image by global_load_lds into a ring of THREE step buffers, fetched TWO steps ahead, one
//           barrier per step (see the loop); `big` / `small` accumulators as in the convolution kernel; epilogue: [exact rescale,] bias
//           [+ second bias], [ReLU, min(20)], [skip sum with LayerNorm on skip0], store (bf16: ONE rounding) -- or the fp32 time-major
//           store of the LSTM gates, staged through LDS so that a store instruction writes whole 256-byte row segments.
#include "storage.h"

namespace nbasr {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 pw_h2 __attribute__((ext_vector_type(2)));

constexpr int PW_M = 128, PW_N = 256, PW_K = 32;                 // tile and K-step
constexpr int PW_THREADS = 512;

// one element of either activation storage type; the bf16 store is the ONE rounding of a result
__device__ __forceinline__ float pw_load(const float* p) { return *p; }
__device__ __forceinline__ float pw_load(const bf16_t* p) { return __uint_as_float(static_cast<unsigned>(p->bits) << 16); }
__device__ __forceinline__ void pw_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void pw_store(bf16_t* p, float v) { p->bits = static_cast<unsigned short>(pack_bf16x2(v, 0.f) & 0xffffu); }

// ---- the operand schemes: what really differs ----------------------------------------------------------------------------------
template <int TERMS>
struct PwSteps {
    static constexpr int NS = TERMS;
    static constexpr int A_STEP = TERMS * 2 * 2 * PW_M * 16;     // [split][block][half][128 rows][8 ch]: 16 / 8 KiB
    static constexpr int X_STEP = TERMS * 2 * 2 * PW_N * 16;     // [split][block][half][256 frames][8 ch]: 32 / 16 KiB
    static constexpr int RING = 3;                               // step buffers: the one being multiplied + two in flight
    static constexpr int LDS = RING * (A_STEP + X_STEP);         // 144 / 72 KiB (of 160 per compute unit)
    static constexpr int DMA_PER_WAVE = 3 * TERMS;               // LDS-DMA instructions of one wave per K-step
};

struct PwF16x2 : PwSteps<2> {
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    typedef float act_t;
    static constexpr bool SCALED = true;                         // per-row weight scales, per-(utterance, frame tile) inverse scale
    static constexpr bool ORDER_BY_HOST = true;                  // m-major or n-major tiles, chosen in pw_run
    static constexpr int LD_ALIGN = 4, PROJECTION_LD_ALIGN = 1;  // the projection takes fp32 rows at any pitch (the backward's column matrices)
    // two (already scaled) values -> one dword per term: (hi, hi), (lo', lo') with lo' = (v - hi) 2^11 -- NOT SplitF16x2::split, whose low
    // term stays unscaled
    __device__ static __forceinline__ void split2(float a, float b, unsigned (&d)[NS]) {
        const _Float16 ha = static_cast<_Float16>(a), hb = static_cast<_Float16>(b);
        d[0] = __builtin_bit_cast(unsigned, pw_h2{ha, hb});
        d[1] = __builtin_bit_cast(unsigned, pw_h2{static_cast<_Float16>((a - static_cast<float>(ha)) * 2048.f),
                                                  static_cast<_Float16>((b - static_cast<float>(hb)) * 2048.f)});
    }
    __device__ static __forceinline__ floatx4 mfma(vec8 a, vec8 b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

struct PwBf16 : PwSteps<1> {
    typedef __bf16 vec8 __attribute__((ext_vector_type(8)));
    typedef bf16_t act_t;
    static constexpr bool SCALED = false;
    static constexpr bool ORDER_BY_HOST = false;                 // always frame-tile-major
    static constexpr int LD_ALIGN = 8, PROJECTION_LD_ALIGN = 8;  // bf16 rows are pitched to 16 bytes
    __device__ static __forceinline__ void split2(float a, float b, unsigned (&d)[NS]) { d[0] = pack_bf16x2(a, b); }
    __device__ static __forceinline__ floatx4 mfma(vec8 a, vec8 b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

__host__ __device__ inline void pw_pow2(float absmax, int target, float& scale, float& inv)
{
    unsigned bits;
    __builtin_memcpy(&bits, &absmax, 4);
    const int e = static_cast<int>((bits >> 23) & 0xffu);
    int k = (bits & 0x7fffffffu) ? (127 + target) - e : 0;
    k = k > 126 ? 126 : (k < -126 ? -126 : k);
    const unsigned sb = static_cast<unsigned>(127 + k) << 23, ib = static_cast<unsigned>(127 - k) << 23;
    __builtin_memcpy(&scale, &sb, 4);
    __builtin_memcpy(&inv, &ib, 4);
}

// ---- weights (scaled scheme: per-row 2^kw and 2^-kw behind the images) -----------------------------------------------------------
__global__ __launch_bounds__(256) void pw_row_scales_kernel(const float* __restrict__ w, float* __restrict__ scales, int c_out,
                                                            int c_in, int rows)
{
    __shared__ float s_max[4];
    const int co = blockIdx.x;
    float m = 0.f;
    if (co < c_out)
        for (int i = threadIdx.x; i < c_in; i += 256) m = fmaxf(m, fabsf(w[static_cast<size_t>(co) * c_in + i]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float scale, inv;
        pw_pow2(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3])), 13, scale, inv);
        scales[co] = scale;
        scales[rows + co] = inv;
    }
}

template <class P>
__global__ __launch_bounds__(256) void pw_pack_weights_kernel(const float* __restrict__ w, unsigned short* __restrict__ wp,
                                                              const float* __restrict__ row_scale, int c_out, int c_in,
                                                              int n_mt, int n_ks)
{
    const long long total = static_cast<long long>(n_mt) * n_ks * PW_M * PW_K;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += static_cast<long long>(gridDim.x) * blockDim.x) {
        long long e = i;
        const int ci_l = e % PW_K; e /= PW_K;
        const int co_l = e % PW_M; e /= PW_M;
        const int ks = e % n_ks; e /= n_ks;
        const int mt = static_cast<int>(e);
        const int co = mt * PW_M + co_l, ci = ks * PW_K + ci_l;
        float v = 0.f;
        if (co < c_out && ci < c_in) v = P::SCALED ? w[static_cast<size_t>(co) * c_in + ci] * row_scale[co] : w[static_cast<size_t>(co) * c_in + ci];
        unsigned d[P::NS];
        P::split2(v, 0.f, d);
        const int blk = ci_l >> 4, half = (ci_l >> 3) & 1, c8 = ci_l & 7;
        const size_t step = static_cast<size_t>(mt) * n_ks + ks;
        const size_t base = step * (P::A_STEP / 2) + ((static_cast<size_t>(blk) * 2 + half) * PW_M + co_l) * 8 + c8;
#pragma unroll
        for (int s = 0; s < P::NS; ++s) wp[base + s * (P::A_STEP / 2 / P::NS)] = static_cast<unsigned short>(d[s] & 0xffffu);   // split s = s-th part of the step image
    }
}

// ---- the operand image ------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per (frame tile, K-step, utterance), lane = frame -- thousands of light workgroups whose loads are all
// issued up front, instead of one 1024-thread workgroup per tile that walked the channels in a latency-bound loop (116 us for the
// LSTM projection's 77 MB at 64 x 250 frames, the same 103 us at 8 x 250).  The scaled scheme takes two launches:
//   pw_tile_max_kernel  partial[(b * n_nt + nt) * n_ks + ks] = max |x| over the 32 channels x 256 frames of the K-step
//   pw_presplit_kernel  reduces the tile's n_ks partials (exact whatever the order), scales, splits and writes the image
//                       rows of its K-step (16 B per lane, lanes along frames: 1 KiB contiguous per wave store);
//                       inv_scale[b * n_nt + nt] = 2^-k of the tile;
// the bf16 scheme only the second, which rounds to bf16 (with LNX: what the reference's LayerNorm module returns under
// model.to(bfloat16)).

// the 32 channels of this workgroup's K-step at this lane's frame, the pending LayerNorm applied in fp32 (zero outside the tensor)
template <bool LNX, class T>
__device__ __forceinline__ void pw_fetch32(const T* __restrict__ x, int c_in, int frames, int ld, const LnRef& ln, float (&v)[PW_K])
{
    const int ci0 = blockIdx.y * PW_K, b = blockIdx.z;
    const int t = blockIdx.x * PW_N + threadIdx.x;
    const bool live = t < frames;
    const T* __restrict__ xb = x + static_cast<size_t>(b) * c_in * ld + t;
    float mean = 0.f, rstd = 0.f;
    if (LNX && live) {
        const float* st = ln.stats + static_cast<size_t>(b) * 2 * ld;
        mean = st[t]; rstd = st[ld + t];
    }
#pragma unroll
    for (int c = 0; c < PW_K; ++c) {
        const int ci = ci0 + c;                                  // wave-uniform
        v[c] = (live && ci < c_in) ? pw_load(xb + static_cast<size_t>(ci) * ld) : 0.f;
    }
    if (LNX) {
#pragma unroll
        for (int c = 0; c < PW_K; ++c) {
            const int ci = ci0 + c;
            if (live && ci < c_in) v[c] = ln_apply(v[c], mean, rstd, ln.gamma[ci], ln.beta[ci]);
        }
    }
}

template <bool LNX>
__global__ __launch_bounds__(256) void pw_tile_max_kernel(const float* __restrict__ x, float* __restrict__ partial, int c_in,
                                                          int frames, int ld, int n_ks, const LnRef ln)
{
    __shared__ float s_max[4];
    float v[PW_K];
    pw_fetch32<LNX>(x, c_in, frames, ld, ln, v);
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < PW_K; ++c) m = fmaxf(m, fabsf(v[c]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        partial[(static_cast<size_t>(blockIdx.z) * gridDim.x + blockIdx.x) * n_ks + blockIdx.y] = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
}

// `inv_scale` and `partial` are read and written by the scaled scheme only
template <class P, bool LNX>
__global__ __launch_bounds__(256) void pw_presplit_kernel(const typename P::act_t* __restrict__ x, unsigned char* __restrict__ image,
                                                          float* __restrict__ inv_scale, const float* __restrict__ partial,
                                                          int c_in, int frames, int ld, int n_ks, const LnRef ln)
{
    const int nt = blockIdx.x, ks = blockIdx.y, b = blockIdx.z;
    const int lane_t = threadIdx.x;                          // frame within the tile
    float v[PW_K];
    pw_fetch32<LNX>(x, c_in, frames, ld, ln, v);
    float scale = 1.f;
    if constexpr (P::SCALED) {
        // the tile's maximum: every wave reduces the n_ks partials on its own (no barrier)
        const float* __restrict__ pt = partial + (static_cast<size_t>(b) * gridDim.x + nt) * n_ks;
        float tile_max = 0.f;
        for (int i = threadIdx.x & 63; i < n_ks; i += 64) tile_max = fmaxf(tile_max, pt[i]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) tile_max = fmaxf(tile_max, __shfl_xor(tile_max, d));
        float inv;
        pw_pow2(tile_max, 14, scale, inv);
        if (threadIdx.x == 0 && ks == 0) inv_scale[static_cast<size_t>(b) * gridDim.x + nt] = inv;
    }
    unsigned char* step = image + ((static_cast<size_t>(b) * gridDim.x + nt) * n_ks + ks) * P::X_STEP;
#pragma unroll
    for (int bh = 0; bh < 4; ++bh) {                         // (16-channel block, 8-channel half)
        u4v term[P::NS];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v0 = v[bh * 8 + 2 * q], v1 = v[bh * 8 + 2 * q + 1];
            unsigned d[P::NS];
            if constexpr (P::SCALED) P::split2(v0 * scale, v1 * scale, d);
            else P::split2(v0, v1, d);
#pragma unroll
            for (int s = 0; s < P::NS; ++s) term[s][q] = d[s];
        }
        unsigned char* row = step + (bh * PW_N + lane_t) * 16;
#pragma unroll
        for (int s = 0; s < P::NS; ++s) *reinterpret_cast<u4v*>(row + s * (P::X_STEP / P::NS)) = term[s];
    }
}

// ---- the GEMM -----------------------------------------------------------------------------------------------------------------
template <class P>
struct PointwiseArgs {
    const unsigned char* image; const float* x_inv; const unsigned char* wp; const float* w_inv;      // x_inv, w_inv: scaled scheme
    const float* bias; const float* bias2;
    const typename P::act_t* s0; const typename P::act_t* s1; const typename P::act_t* s2;
    void* y;                                 // SWAP: float (frames, rows of utterances, c_out); else act_t (batch, c_out, ld)
    int c_out, frames, ld_out, n_ks, n_mt, n_nt, batch;
    int n_major;                             // tile order (see the kernel)
    int row_stride_t, row_stride_b;          // SWAP store: y[(t * row_stride_t + b * row_stride_b) * c_out + m]
    LnRef ln_s0;
};

template <class P, bool SWAP, bool RELU>
__global__ __launch_bounds__(PW_THREADS, 2) void pw_gemm_kernel(const PointwiseArgs<P> a)
{
    typedef typename P::vec8 vec8;
    typedef typename P::act_t act_t;
    constexpr int NS = P::NS, A_STEP = P::A_STEP, X_STEP = P::X_STEP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const Abuf = smem;                       // [RING][A_STEP]
    unsigned char* const Xbuf = smem + P::RING * A_STEP;    // [RING][X_STEP]

    // XCD-aware tile order: every XCD takes a contiguous run of the linear tile index L, dispatched in order.
    //  m-major (rounds 1-2): L = (mt, b, nt) -- an XCD keeps ONE or two weight tiles in its L2 and streams the whole operand image
    //    past them once per row tile: n_mt passes over the image in all (LSTM projection: 16 x 77 MB; measured 1.45 GB of fabric
    //    reads per launch for 215 MB of algorithmic bytes, at 0.40 matrix-pipe occupancy -- VERDICT r2 weak 6);
    //  n-major (round 3, chosen by the host when the packed weights are the smaller operand -- always for K <= 1200; the bf16 scheme
    //    knows no other): L = (b, nt, mt)
    //    -- the workgroups an XCD runs at once are ALL row tiles of a few frame tiles: the frame tiles' image (1.2 MB each) sits in
    //    the XCD's L2 for its n_mt readers and the (9.6 MB) weights stream from the last-level cache: one pass over the image.
    // Same tiles, same sums: the order changes nothing in the results.
    const int nwg = gridDim.x, id = blockIdx.x;
    const int xq = nwg >> 3, xr = nwg & 7, xcd = id & 7;
    const int L = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (id >> 3);
    int mt_i, b, nt_i;
    if (!P::ORDER_BY_HOST || a.n_major) {
        const int ntg = L / a.n_mt;
        mt_i = L - ntg * a.n_mt;
        b = ntg / a.n_nt;
        nt_i = ntg - b * a.n_nt;
    } else {
        const int per_m = a.n_nt * a.batch;
        mt_i = L / per_m;
        const int rem = L - mt_i * per_m;
        b = rem / a.n_nt;
        nt_i = rem - b * a.n_nt;
    }
    const int m0 = mt_i * PW_M, n0 = nt_i * PW_N;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int l15 = lane & 15, kq = lane >> 4;
    const bool wave_active = (m0 + wm * 64) < a.c_out && (n0 + wn * 64) < a.ld_out;

    const unsigned char* __restrict__ wsrc = a.wp + static_cast<size_t>(mt_i) * a.n_ks * A_STEP;
    const unsigned char* __restrict__ xsrc = a.image + (static_cast<size_t>(b) * a.n_nt + nt_i) * a.n_ks * X_STEP;

    floatx4 big[4][4], small[4][4];                         // `small` (the two cross terms of the split) is dead for one term
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { big[i][j][r] = 0.f; small[i][j][r] = 0.f; }

    // one K-step = NS x (8 weights + 16 image) 1 KiB LDS-DMA pieces, 3 NS per wave
    auto dma_step = [&](int ks, int buf) {
        const unsigned char* ws = wsrc + static_cast<size_t>(ks) * A_STEP;
        const unsigned char* xs = xsrc + static_cast<size_t>(ks) * X_STEP;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int piece = wave * NS + j;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ws + piece * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) void*)(Abuf + buf * A_STEP + piece * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 2 * NS; ++j) {
            const int piece = wave * 2 * NS + j;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xs + piece * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) void*)(Xbuf + buf * X_STEP + piece * 1024), 16, 0, 0);
        }
    };

    // per-lane fragment bases: k quarter kq -> 16-channel block kq >> 1, 8-channel half kq & 1
    const int a_lane = ((kq * PW_M) + wm * 64 + l15) * 16;
    const int x_lane = ((kq * PW_N) + wn * 64 + l15) * 16;

    // One K-step of this wave's 64 x 64 tile on step buffer `buf`.  The fragment reads are software-pipelined in place (as mma_step of
    // gemm_conv_split.hip): the A fragments of row block i + 1 are read behind the first MFMA block of row block i, so only the first
    // reads of a step wait on LDS latency.  Every accumulator sees the MFMAs it always saw, in the same order (`small`: lo * hi, then
    // hi * lo; `big`: hi * hi; ks ascending): the sums are the same bit for bit.
    auto mma_step = [&](int buf) {
        const unsigned char* A = Abuf + buf * A_STEP + a_lane;
        const unsigned char* X = Xbuf + buf * X_STEP + x_lane;
        auto read_a = [&](int i, vec8 (&f)[NS]) {
#pragma unroll
            for (int s = 0; s < NS; ++s) f[s] = *reinterpret_cast<const vec8*>(A + s * (A_STEP / NS) + i * 16 * 16);
        };
        vec8 bt[4][NS], at[2][NS];                          // terms: [0] = hi (or the value), [1] = lo
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int s = 0; s < NS; ++s) bt[j][s] = *reinterpret_cast<const vec8*>(X + s * (X_STEP / NS) + j * 16 * 16);
        read_a(0, at[0]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (NS == 2) {
                    floatx4 c = small[i][j];
                    c = P::mfma(at[i & 1][1], bt[j][0], c);
                    c = P::mfma(at[i & 1][0], bt[j][1], c);
                    small[i][j] = c;
                }
                big[i][j] = P::mfma(at[i & 1][0], bt[j][0], big[i][j]);
                __builtin_amdgcn_sched_barrier(0);
                if (j == 0 && i < 3) read_a(i + 1, at[(i + 1) & 1]);      // behind the first block: 9 (3) MFMAs to land
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- main loop: ONE barrier per K-step, operands fetched TWO steps ahead -----------------------------------------------------------
    // A step multiplies for ~0.65 us at the matrix pipe's rate, an LDS-DMA piece that misses the L2 (the weights always do under the
    // n-major order) takes longer than that to land; fetched one step ahead and waited for at the end of that step, the DMA's
    // latency set the step time.  A K-step of 64 k would hide it as well, but two double steps of the split scheme are 192 KiB; a
    // ring of THREE single steps (144 KiB) gives the same two steps of flight.
    //   step ks:  DMA of step ks + 2 -> buffer (ks + 2) % 3;  MFMAs on buffer ks % 3;
    //             wait until this wave's DMA of step ks + 1 has landed (the newest batch may stay in flight: loads retire in order,
    //             so vmcnt(DMA_PER_WAVE) leaves only step ks + 2 outstanding);  barrier.
    // Hazards.  Read after fill: buffer (ks + 1) % 3 is read in step ks + 1 only, i.e. behind the barrier that ends step ks, which
    // every wave reaches only after the counted wait for its own pieces of step ks + 1 -- all 8 waves' pieces have landed.  Fill after
    // read: buffer (ks + 2) % 3 = (ks - 1) % 3 was last read in step ks - 1; its refill is issued inside step ks, behind the barrier that
    // ended step ks - 1, and every wave's fragment reads of a step have RETURNED before that barrier (the MFMAs consumed them, and the
    // wait in front of the barrier names lgkmcnt(0)) -- in either phase order below.  The barrier is the bare instruction: the fence of
    // __syncthreads() would drain vmcnt to 0 and with it the second step of flight.
    // Waves 0-3 and 4-7 share the four SIMDs pairwise.  As in gemm_conv_split.hip the two halves run a step in OPPOSITE order: the older
    // wave issues its DMA first and multiplies last, the younger one multiplies first (at s_setprio 1, so that it really gets the pipe)
    // and issues last -- each wave's ~1 500 cycles of DMA issue sit beside its partner's MFMAs.
    const bool older = wave < 4;
    const int n_ks = a.n_ks;
    dma_step(0, 0);
    if (n_ks > 1) {
        dma_step(1, 1);
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" :: "n"(P::DMA_PER_WAVE) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (!older) __builtin_amdgcn_s_setprio(1);
    int buf = 0;
#pragma unroll 1
    for (int ks = 0; ks < n_ks; ++ks) {
        const bool ahead = ks + 2 < n_ks;                   // there is a step after the next: fetch it
        const int fill = buf == 0 ? 2 : buf - 1;            // (ks + 2) % RING
        if (older && ahead) dma_step(ks + 2, fill);
        if (wave_active) mma_step(buf);
        if (!older && ahead) dma_step(ks + 2, fill);
        if (ahead) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(P::DMA_PER_WAVE) : "memory");
        else       asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        buf = buf == 2 ? 0 : buf + 1;
    }
    if (!older) __builtin_amdgcn_s_setprio(0);

    if (!wave_active) return;
    float x_inv = 1.f;
    if constexpr (P::SCALED) x_inv = a.x_inv[static_cast<size_t>(b) * a.n_nt + nt_i];
    // element r of MFMA tile (i, j), row m, before the bias: the terms joined and the two operand scales undone (all exact)
    auto product = [&](int i, int j, int r, int m) {
        float v = big[i][j][r];
        if constexpr (NS == 2) v += small[i][j][r] * (1.f / 2048.f);
        if constexpr (P::SCALED) v = v * x_inv * a.w_inv[m];
        return v;
    };
    if constexpr (SWAP) {
        // Time-major store, through LDS.  Straight from the accumulators a store instruction wrote 16 rows x 64 bytes (a lane holds 4
        // consecutive m of ONE frame, the rows of y are c_out floats apart); staged, it writes 4 rows x 256 bytes: 64 consecutive m of one
        // (t, b) row per 16 lanes x 16 bytes.  A wave stages one 16-frame column block of its tile at a time -- 16 rows x 64 m fp32, row
        // stride 68 floats (the 8 lanes of a ds_write_b128 group land on 8 x 4 different banks) = 4.25 KiB of the operand buffers,
        // which nobody reads or fills any more: the loop's last barrier stood behind every wave's last reads and its vmcnt(0).  The
        // tile is wave-private, so the passes need no barrier, only the wave's own LDS counter.  Values are computed exactly as before.
        constexpr int TS = 64 + 4;
        static_assert(8 * 16 * TS * 4 <= P::LDS, "output staging must fit the operand buffers");
        float* const T = reinterpret_cast<float*>(smem) + wave * (16 * TS);
        const int mseg = m0 + wm * 64 + l15 * 4;            // copy-out: this lane's 4 consecutive m
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mb = m0 + wm * 64 + i * 16 + kq * 4;
                floatx4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = mb + r;
                    float v = 0.f;
                    if (m < a.c_out) {
                        v = product(i, j, r, m) + a.bias[m];
                        if (a.bias2) v += a.bias2[m];
                        if (RELU) v = relu_clamp(v);
                    }
                    o[r] = v;
                }
                *reinterpret_cast<floatx4*>(T + l15 * TS + i * 16 + kq * 4) = o;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's tile is written (and the reads below stay below)
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int row = it * 4 + kq;
                const int n = n0 + wn * 64 + j * 16 + row;
                if (n >= a.frames || mseg >= a.c_out) continue;
                const floatx4 o = *reinterpret_cast<const floatx4*>(T + row * TS + l15 * 4);
                float* dst = static_cast<float*>(a.y) + (static_cast<size_t>(n) * a.row_stride_t + static_cast<size_t>(b) * a.row_stride_b) * a.c_out + mseg;
                *reinterpret_cast<floatx4*>(dst) = o;           // c_out = 4 hidden with hidden % 4 == 0 (pw_projection): a quad is inside or outside as a whole
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads have returned before the next pass overwrites the tile
        }
        return;
    }
    // the `linear` node: bias, ReLU, min(20), the skips, straight from the accumulators (rows of y are frame-contiguous)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + l15;
            const int mb = m0 + wm * 64 + i * 16 + kq * 4;
            if (n >= a.ld_out) continue;
            const bool live = n < a.frames;
            float s0m = 0.f, s0r = 0.f;
            if (a.s0 && a.ln_s0.stats) {
                const float* st = a.ln_s0.stats + static_cast<size_t>(b) * 2 * a.ld_out;
                s0m = st[n]; s0r = st[a.ld_out + n];
            }
            act_t* yb = static_cast<act_t*>(a.y);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mb + r;
                if (m >= a.c_out) continue;
                float v = product(i, j, r, m) + a.bias[m];
                if (RELU) v = relu_clamp(v);
                const size_t off = (static_cast<size_t>(b) * a.c_out + m) * a.ld_out + n;
                // the skips in python's sum order, in fp32; ONE rounding (as the bf16 node kernels: grouped_conv_impl.h)
                if (a.s0) v += a.ln_s0.stats ? ln_apply(pw_load(a.s0 + off), s0m, s0r, a.ln_s0.gamma[m], a.ln_s0.beta[m]) : pw_load(a.s0 + off);
                if (a.s1) v += pw_load(a.s1 + off);
                if (a.s2) v += pw_load(a.s2 + off);
                pw_store(yb + off, live ? v : 0.f);
            }
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static inline int pw_n_ks(int c_in) { return (c_in + PW_K - 1) / PW_K; }
static inline int pw_n_mt(int c_out) { return (c_out + PW_M - 1) / PW_M; }
static inline int pw_n_nt(int ld) { return (ld + PW_N - 1) / PW_N; }
static inline size_t pw_round4(size_t n) { return (n + 3) & ~static_cast<size_t>(3); }
template <class P> static size_t pw_image_bytes(int batch, int c_in, int ld) { return static_cast<size_t>(batch) * pw_n_nt(ld) * pw_n_ks(c_in) * P::X_STEP; }
template <class P> static size_t pw_weight_image_bytes(int c_out, int c_in) { return static_cast<size_t>(pw_n_mt(c_out)) * pw_n_ks(c_in) * P::A_STEP; }

template <class P>
static size_t pw_weights_bytes(int c_out, int c_in)
{
    if (c_out <= 0 || c_in <= 0) return 0;
    return pw_weight_image_bytes<P>(c_out, c_in) + (P::SCALED ? 2 * static_cast<size_t>(pw_n_mt(c_out)) * PW_M * sizeof(float) : 0);
}

template <class P>
static size_t pw_workspace_bytes(int batch, int c_in, int ld)
{
    if (batch <= 0 || c_in <= 0 || ld <= 0) return 0;
    // operand image; scaled: + one inverse scale per (utterance, frame tile), one partial maximum per (utterance, frame tile, K-step)
    const size_t tiles = static_cast<size_t>(batch) * pw_n_nt(ld);
    return pw_image_bytes<P>(batch, c_in, ld) + (P::SCALED ? (pw_round4(tiles) + tiles * pw_n_ks(c_in)) * sizeof(float) : 0);
}

template <class P>
static int pw_pack(const char* what, const float* w, void* packed, int c_out, int c_in, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(c_out > 0 && c_in > 0, NBASR_EINVAL, "%s: bad sizes", what);
    NBASR_REQUIRE(w && packed, NBASR_ENULL, "%s: NULL pointer", what);
    NBASR_REQUIRE(aligned16(packed), NBASR_EALIGN, "%s: packed buffer must be 16-byte aligned", what);
    const int n_mt = pw_n_mt(c_out), n_ks = pw_n_ks(c_in);
    float* scales = nullptr;
    if (P::SCALED) {
        scales = reinterpret_cast<float*>(static_cast<unsigned char*>(packed) + pw_weight_image_bytes<P>(c_out, c_in));
        hipLaunchKernelGGL(pw_row_scales_kernel, dim3(n_mt * PW_M), dim3(256), 0, as_stream(stream), w, scales, c_out, c_in, n_mt * PW_M);
    }
    hipLaunchKernelGGL(pw_pack_weights_kernel<P>, dim3(1024), dim3(256), 0, as_stream(stream), w, static_cast<unsigned short*>(packed), scales,
                       c_out, c_in, n_mt, n_ks);
    return launch_status(what);
}

// x -> the operand image in ws (scaled: then batch * n_nt inverse scales and the partial maxima); `ln` = pending LayerNorm of x
template <class P, bool LNX>
static int pw_image(const typename P::act_t* x, void* ws, int batch, int c_in, int frames, int ld, LnRef ln, hipStream_t stream, const char* what)
{
    unsigned char* image = static_cast<unsigned char*>(ws);
    float* inv = nullptr;
    float* partial = nullptr;
    const int n_ks = pw_n_ks(c_in);
    const dim3 grid(pw_n_nt(ld), n_ks, batch);              // utterances on grid z: pw_checks holds batch <= 65535
    if constexpr (P::SCALED) {
        inv = reinterpret_cast<float*>(image + pw_image_bytes<P>(batch, c_in, ld));
        partial = inv + pw_round4(static_cast<size_t>(batch) * pw_n_nt(ld));
        hipLaunchKernelGGL(pw_tile_max_kernel<LNX>, grid, dim3(256), 0, stream, x, partial, c_in, frames, ld, n_ks, ln);
    }
    hipLaunchKernelGGL((pw_presplit_kernel<P, LNX>), grid, dim3(256), 0, stream, x, image, inv, partial, c_in, frames, ld, n_ks, ln);
    return launch_status(what);
}

static int pw_checks(const char* what, const void* x, const void* ws, const void* packed_w, const float* bias, const void* y,
                     int batch, int c_in, int frames, int ld, int c_out)
{
    NBASR_REQUIRE(batch >= 0 && c_in > 0 && c_out > 0 && frames >= 0 && ld >= frames, NBASR_EINVAL, "%s: bad sizes", what);
    if (batch == 0 || frames == 0) return 1;
    NBASR_REQUIRE(batch <= 65535, NBASR_EINVAL, "%s: batch %d > 65535", what, batch);
    NBASR_REQUIRE(x && ws && packed_w && bias && y, NBASR_ENULL, "%s: x, workspace, packed_w, bias, y must be non-NULL", what);
    NBASR_REQUIRE(aligned16(ws) && aligned16(packed_w), NBASR_EALIGN, "%s: workspace and packed weights must be 16-byte aligned", what);
    return NBASR_OK;
}

// the image pass and the GEMM of a checked call; `a` arrives with the epilogue's operands (biases, skips, y, strides, ln_s0)
template <class P, bool SWAP, bool RELU>
static int pw_run(const char* what, const typename P::act_t* x, void* ws, const void* packed_w, PointwiseArgs<P> a, int batch, int c_in,
                  int frames, int ld, int c_out, LnRef ln_x, hipStream_t stream)
{
    const int rc = ln_x.stats ? pw_image<P, true>(x, ws, batch, c_in, frames, ld, ln_x, stream, what)
                              : pw_image<P, false>(x, ws, batch, c_in, frames, ld, ln_x, stream, what);
    if (rc != NBASR_OK) return rc;
    a.image = static_cast<const unsigned char*>(ws);
    a.wp = static_cast<const unsigned char*>(packed_w);
    a.n_mt = pw_n_mt(c_out); a.n_ks = pw_n_ks(c_in); a.n_nt = pw_n_nt(ld);
    if (P::SCALED) {
        a.x_inv = reinterpret_cast<const float*>(a.image + pw_image_bytes<P>(batch, c_in, ld));
        a.w_inv = reinterpret_cast<const float*>(a.wp + pw_weight_image_bytes<P>(c_out, c_in)) + static_cast<size_t>(a.n_mt) * PW_M;
    }
    a.c_out = c_out; a.frames = frames; a.ld_out = ld; a.batch = batch;

    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(pw_gemm_kernel<P, SWAP, RELU>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, P::LDS);
    if (attr != hipSuccess) {
        set_error("%s: cannot reserve %d bytes of LDS: %s", what, P::LDS, hipGetErrorString(attr));
        return static_cast<int>(attr);
    }
    const long long nwg = static_cast<long long>(a.n_mt) * a.n_nt * a.batch;
    NBASR_REQUIRE(nwg < (1ll << 31), NBASR_EINVAL, "%s: too many tiles (%lld)", what, nwg);
    // tile order: stream the SMALLER operand (per K-step a row tile costs A_STEP bytes of weights, a frame tile X_STEP of image)
    // (A/B on the LSTM projection, 64 x 250 frames: 1.45 GB -> 0.56 GB of HBM traffic per launch, 254 -> 248 us; throughput equal within noise)
    // (a scheme that is always n-major ignores the choice)
    a.n_major = static_cast<long long>(a.n_mt) * P::A_STEP <= static_cast<long long>(a.n_nt) * a.batch * P::X_STEP ? 1 : 0;
    hipLaunchKernelGGL((pw_gemm_kernel<P, SWAP, RELU>), dim3(static_cast<unsigned>(nwg)), dim3(PW_THREADS), P::LDS, stream, a);
    return launch_status(what);
}

template <class P>
static int pw_linear(const char* what, const typename P::act_t* x, void* ws, const void* packed_w, const float* bias,
                     const typename P::act_t* skip0, const typename P::act_t* skip1, const typename P::act_t* skip2, typename P::act_t* y,
                     int batch, int c_in, int frames, int ld, int c_out, const nbasr_deferred_ln* ln, int ln_on_x, int ln_on_skip0,
                     nbasr_stream_t stream)
{
    clear_error();
    const int rc0 = pw_checks(what, x, ws, packed_w, bias, y, batch, c_in, frames, ld, c_out);
    if (rc0 != NBASR_OK) return rc0 == 1 ? NBASR_OK : rc0;
    NBASR_REQUIRE(ld % P::LD_ALIGN == 0, NBASR_EALIGN, "%s: ld=%d must be a multiple of %d (rows are pitched to 16 bytes)", what, ld, P::LD_ALIGN);
    const bool any_ln = ln && (ln_on_x || (ln_on_skip0 && skip0));
    NBASR_REQUIRE(!any_ln || (ln->stats && ln->gamma && ln->beta), NBASR_ENULL, "%s: deferred LayerNorm needs stats, gamma and beta", what);
    NBASR_REQUIRE(!(ln && ln_on_x && ln_on_skip0 && skip0) || c_in == c_out, NBASR_EINVAL, "%s: one descriptor for x and skip0 needs equal shapes", what);
    PointwiseArgs<P> a{};
    a.bias = bias; a.s0 = skip0; a.s1 = skip1; a.s2 = skip2; a.y = y;
    a.ln_s0 = ln_ref(ln, ln_on_skip0 != 0 && skip0 != nullptr);
    return pw_run<P, false, true>(what, x, ws, packed_w, a, batch, c_in, frames, ld, c_out, ln_ref(ln, ln_on_x != 0), as_stream(stream));
}

// gates_ws[(t * batch_total + batch_offset + b) * 4 hidden + j]; the caller has cleared the error text
template <class P>
static int pw_projection(const char* what, const typename P::act_t* x, void* ws, const void* packed_w_ih, const float* b_ih, const float* b_hh,
                         float* gates_ws, int batch, int c_in, int frames, int ld, int hidden, const nbasr_deferred_ln* ln, int batch_total,
                         int batch_offset, nbasr_stream_t stream)
{
    const int rc0 = pw_checks(what, x, ws, packed_w_ih, b_ih, gates_ws, batch, c_in, frames, ld, 4 * hidden);
    if (rc0 != NBASR_OK) return rc0 == 1 ? NBASR_OK : rc0;
    NBASR_REQUIRE(b_hh != nullptr, NBASR_ENULL, "%s: b_hh is NULL", what);
    NBASR_REQUIRE(hidden % 4 == 0 && aligned16(gates_ws) && ld % P::PROJECTION_LD_ALIGN == 0, NBASR_EALIGN,
                  "%s: hidden %% 4, ld %% %d and 16-byte aligned gates_ws required", what, P::PROJECTION_LD_ALIGN);
    NBASR_REQUIRE(!ln || (ln->stats && ln->gamma && ln->beta), NBASR_ENULL, "%s: deferred LayerNorm needs stats, gamma and beta", what);
    PointwiseArgs<P> a{};
    a.bias = b_ih; a.bias2 = b_hh; a.y = gates_ws + static_cast<size_t>(batch_offset) * 4 * hidden;
    a.row_stride_t = batch_total; a.row_stride_b = 1;
    return pw_run<P, true, false>(what, x, ws, packed_w_ih, a, batch, c_in, frames, ld, 4 * hidden, ln_ref(ln, true), as_stream(stream));
}

}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_pointwise_packed_weights_bytes(int c_out, int c_in) { return pw_weights_bytes<PwF16x2>(c_out, c_in); }
extern "C" size_t nbasr_pointwise_bf16_weights_bytes(int c_out, int c_in) { return pw_weights_bytes<PwBf16>(c_out, c_in); }
extern "C" size_t nbasr_pointwise_workspace_bytes(int batch, int c_in, int ld) { return pw_workspace_bytes<PwF16x2>(batch, c_in, ld); }
extern "C" size_t nbasr_pointwise_bf16_workspace_bytes(int batch, int c_in, int ld) { return pw_workspace_bytes<PwBf16>(batch, c_in, ld); }

extern "C" int nbasr_pack_pointwise_weights(const float* w, void* packed, int c_out, int c_in, nbasr_stream_t stream)
{
    return pw_pack<PwF16x2>("nbasr_pack_pointwise_weights", w, packed, c_out, c_in, stream);
}

extern "C" int nbasr_pack_pointwise_weights_bf16(const float* w, void* packed, int c_out, int c_in, nbasr_stream_t stream)
{
    return pw_pack<PwBf16>("nbasr_pack_pointwise_weights_bf16", w, packed, c_out, c_in, stream);
}

extern "C" int nbasr_linear_fused_packed(const float* x, void* ws, const void* packed_w, const float* bias, const float* skip0,
                                         const float* skip1, const float* skip2, float* y, int batch, int channels_in,
                                         int frames, int ld, int channels_out, const nbasr_deferred_ln* ln, int ln_on_x,
                                         int ln_on_skip0, nbasr_stream_t stream)
{
    return pw_linear<PwF16x2>("nbasr_linear_fused_packed", x, ws, packed_w, bias, skip0, skip1, skip2, y, batch, channels_in, frames, ld,
                              channels_out, ln, ln_on_x, ln_on_skip0, stream);
}

extern "C" int nbasr_linear_fused_bf16(const void* x, void* ws, const void* packed_w, const float* bias, const void* skip0,
                                       const void* skip1, const void* skip2, void* y, int batch, int channels_in, int frames, int ld,
                                       int channels_out, const nbasr_deferred_ln* ln, int ln_on_x, int ln_on_skip0, nbasr_stream_t stream)
{
    return pw_linear<PwBf16>("nbasr_linear_fused_bf16", static_cast<const bf16_t*>(x), ws, packed_w, bias, static_cast<const bf16_t*>(skip0),
                             static_cast<const bf16_t*>(skip1), static_cast<const bf16_t*>(skip2), static_cast<bf16_t*>(y), batch, channels_in,
                             frames, ld, channels_out, ln, ln_on_x, ln_on_skip0, stream);
}

extern "C" int nbasr_lstm_input_projection_packed(const float* x, void* ws, const void* packed_w_ih, const float* b_ih,
                                                  const float* b_hh, float* gates_ws, int batch, int c_in, int frames, int ld,
                                                  int hidden, const nbasr_deferred_ln* ln, nbasr_stream_t stream)
{
    clear_error();
    return pw_projection<PwF16x2>("nbasr_lstm_input_projection_packed", x, ws, packed_w_ih, b_ih, b_hh, gates_ws, batch, c_in, frames, ld, hidden,
                                  ln, batch, 0, stream);
}

extern "C" int nbasr_lstm_input_projection_packed_into(const float* x, void* ws, const void* packed_w_ih, const float* b_ih,
                                                       const float* b_hh, float* gates_ws, int batch, int c_in, int frames, int ld,
                                                       int hidden, const nbasr_deferred_ln* ln, int batch_total, int batch_offset,
                                                       nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(batch_offset >= 0 && batch >= 0 && batch_offset + batch <= batch_total, NBASR_EINVAL,
                  "nbasr_lstm_input_projection_packed_into: utterances %d .. %d do not lie inside a gate tensor of %d", batch_offset,
                  batch_offset + batch, batch_total);
    return pw_projection<PwF16x2>("nbasr_lstm_input_projection_packed", x, ws, packed_w_ih, b_ih, b_hh, gates_ws, batch, c_in, frames, ld, hidden,
                                  ln, batch_total, batch_offset, stream);
}

extern "C" int nbasr_lstm_input_projection_bf16(const void* x, void* ws, const void* packed_w_ih, const float* b_ih, const float* b_hh,
                                                float* gates_ws, int batch, int c_in, int frames, int ld, int hidden,
                                                const nbasr_deferred_ln* ln, nbasr_stream_t stream)
{
    clear_error();
    return pw_projection<PwBf16>("nbasr_lstm_input_projection_bf16", static_cast<const bf16_t*>(x), ws, packed_w_ih, b_ih, b_hh, gates_ws, batch,
                                 c_in, frames, ld, hidden, ln, batch, 0, stream);
}
