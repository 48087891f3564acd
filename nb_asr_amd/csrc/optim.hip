// The optimisation step of the reference's trainer (training/torch/trainer.py:221-225 and :84) over a whole parameter set:
//   the weight-norm regulariser's gradient  g + c_t w,  c_t = coef / ||w_t||   (0.01 * sum(torch.norm(conv.weight)), backward),
//   clip_grad_norm_                         scale = min(1, max_norm / (total_norm + 1e-6)),
//   Adam (no weight decay / amsgrad)        m, v, p updated in the expression order of torch's single-tensor Adam.
// Multi-tensor over a device-resident table (nbasr.h: nbasr_optim_tensor / nbasr_optim_chunk), three launches whatever the tensor
// count, no host synchronisation, no read-back, no floating-point atomics:
//   1. reduce:   one workgroup per chunk; sum g^2 (flagged tensors: also sum g w, sum w^2) in float64 -> partials[chunk][3];
//   2. finalise: ONE workgroup; a wave per tensor sums that tensor's partials (lanes stride over the chunks, then a fixed shuffle
//                tree), lane 0 forms c_t and the tensor's share  sum g^2 + 2 c_t sum g w + c_t^2 sum w^2  of the squared norm of the
//                effective gradient; the shares are added wave by wave, tensor by tensor in table order -> total_norm, scale;
//   3. apply:    one workgroup per chunk; 128-bit loads / stores where p, grad, exp_avg and exp_avg_sq of the tensor are all 16-byte
//                aligned (chunk offsets are multiples of 4 elements), a scalar path otherwise; tails of any length.
// Every sum has a fixed order, so two steps from the same state give the same bits.  grad is only read.
#include "common.h"

namespace nbasr {
namespace {

constexpr int kThreads = 256;

// The table's pointers come out of memory, so the compiler takes them for generic addresses (flat loads): say that they are global.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gfloat4;
__device__ __forceinline__ gfloat* global_ptr(const float* p) { return (gfloat*)p; }
constexpr int kFinalThreads = 1024, kFinalWaves = kFinalThreads / 64;

// The element update is written out operation by operation (no contraction; correctly rounded division and square root, hipcc's
// default): torch's kernels round after each of g.add(w * c), g.mul_(scale), exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2),
// (exp_avg_sq.sqrt() / bc2_sqrt).add_(eps) and p.addcdiv_(exp_avg, denom, value=-step_size); exp_avg.lerp_(g, 1 - beta1) is ATen's
// one fma on the difference.
#pragma clang fp contract(off)
struct Update {
    float c, scale, w1, beta2, w2, eps, neg_step, bc2_sqrt;          // w1 = 1 - beta1, w2 = 1 - beta2, neg_step = -step_size
    bool reg;
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
        if (reg) g = g + p * c;
        g = g * scale;
        const float diff = g - m;                                    // lerp_: the form ATen picks by the weight
        m = w1 < 0.5f ? __builtin_fmaf(w1, diff, m) : __builtin_fmaf(w1 - 1.f, diff, g);
        v = v * beta2;
        v = v + (w2 * g) * g;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = p + (neg_step * m) / denom;
    }
};

__device__ __forceinline__ double wave_sum(double x) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

__global__ __launch_bounds__(kThreads) void optim_reduce_kernel(const nbasr_optim_tensor* __restrict__ tensors,
                                                                const nbasr_optim_chunk* __restrict__ chunks, double* __restrict__ partials)
{
    __shared__ double part[kThreads / 64][3];
    const nbasr_optim_chunk ck = chunks[blockIdx.x];
    const nbasr_optim_tensor t = tensors[ck.tensor];
    const gfloat* __restrict__ g = global_ptr(t.grad) + ck.offset;
    const gfloat* __restrict__ w = global_ptr(t.p) + ck.offset;
    const bool reg = (t.flags & NBASR_OPTIM_WEIGHT_NORM) != 0;
    const int n = ck.length, tid = threadIdx.x;
    double gg = 0.0, gw = 0.0, ww = 0.0;
    const bool vec = ((reinterpret_cast<uintptr_t>(g) | (reg ? reinterpret_cast<uintptr_t>(w) : 0)) & 15u) == 0;
    // Both paths give thread tid the elements 4 i .. 4 i + 3, i = tid, tid + 256, ..., summed in the same expression, then the tail:
    // the partials do not depend on the alignment, to the bit.
    const int n4 = n >> 2;
    const gfloat4* __restrict__ g4 = (const gfloat4*)g;
    const gfloat4* __restrict__ w4 = (const gfloat4*)w;
    for (int i = tid; i < n4; i += kThreads) {
        const f32x4 a = vec ? g4[i] : f32x4{g[4 * i], g[4 * i + 1], g[4 * i + 2], g[4 * i + 3]};
        const double a0 = a.x, a1 = a.y, a2 = a.z, a3 = a.w;
        gg += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        if (reg) {
            const f32x4 b = vec ? w4[i] : f32x4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
            const double b0 = b.x, b1 = b.y, b2 = b.z, b3 = b.w;
            gw += (a0 * b0 + a1 * b1) + (a2 * b2 + a3 * b3);
            ww += (b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3);
        }
    }
    for (int i = (n4 << 2) + tid; i < n; i += kThreads) {
        const double a = g[i];
        gg += a * a;
        if (reg) { const double b = w[i]; gw += a * b; ww += b * b; }
    }
    gg = wave_sum(gg);
    if (reg) { gw = wave_sum(gw); ww = wave_sum(ww); }
    if ((tid & 63) == 0) { part[tid >> 6][0] = gg; part[tid >> 6][1] = gw; part[tid >> 6][2] = ww; }
    __syncthreads();
    if (tid < 3) {
        double s = part[0][tid];
        for (int k = 1; k < kThreads / 64; ++k) s += part[k][tid];
        partials[3 * static_cast<size_t>(blockIdx.x) + tid] = s;
    }
}

__global__ __launch_bounds__(kFinalThreads) void optim_finalize_kernel(const nbasr_optim_tensor* __restrict__ tensors, int n_tensors,
                                                                       const double* __restrict__ partials, float* __restrict__ coefs,
                                                                       float* __restrict__ scale_out, float* __restrict__ total_norm,
                                                                       double coef, double max_norm)
{
    __shared__ double share[kFinalWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double mine = 0.0;                                               // lane 0: this wave's tensors, in table order
    for (int t = wave; t < n_tensors; t += kFinalWaves) {
        const int first = tensors[t].first_chunk, count = tensors[t].n_chunks;
        const bool reg = (tensors[t].flags & NBASR_OPTIM_WEIGHT_NORM) != 0;
        double gg = 0.0, gw = 0.0, ww = 0.0;
        for (int k = lane; k < count; k += 64) {
            const double* __restrict__ q = partials + 3 * static_cast<size_t>(first + k);
            gg += q[0];
            if (reg) { gw += q[1]; ww += q[2]; }
        }
        gg = wave_sum(gg);
        if (reg) { gw = wave_sum(gw); ww = wave_sum(ww); }
        if (lane == 0) {
            double c = 0.0;
            if (reg && coef != 0.0 && ww > 0.0) c = coef / sqrt(ww);   // ||w|| == 0: torch.norm's backward gives a zero gradient
            const float cf = static_cast<float>(c);                   // what apply uses: the norm is that of the gradient it forms
            coefs[t] = cf;
            const double cd = cf;
            mine += gg + 2.0 * cd * gw + cd * cd * ww;
        }
    }
    if (lane == 0) share[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < kFinalWaves; ++k) total += share[k];
        const double norm = sqrt(total < 0.0 ? 0.0 : total);
        *total_norm = static_cast<float>(norm);
        double s = 1.0;
        if (max_norm > 0.0) { s = max_norm / (norm + 1e-6); if (s > 1.0) s = 1.0; }   // (a NaN norm gives a NaN scale, as clip_grad_norm_'s clamp does)
        *scale_out = static_cast<float>(s);
    }
}

__global__ __launch_bounds__(kThreads) void optim_apply_kernel(const nbasr_optim_tensor* __restrict__ tensors,
                                                               const nbasr_optim_chunk* __restrict__ chunks, const float* __restrict__ coefs,
                                                               const float* __restrict__ scale, float w1, float beta2, float w2, float eps)
{
    const nbasr_optim_chunk ck = chunks[blockIdx.x];
    const nbasr_optim_tensor t = tensors[ck.tensor];
    gfloat* __restrict__ p = global_ptr(t.p) + ck.offset;
    const gfloat* __restrict__ g = global_ptr(t.grad) + ck.offset;
    gfloat* __restrict__ m = global_ptr(t.exp_avg) + ck.offset;
    gfloat* __restrict__ v = global_ptr(t.exp_avg_sq) + ck.offset;
    const float c = coefs[ck.tensor];
    const Update up{c, *scale, w1, beta2, w2, eps, -t.step_size, t.bc2_sqrt, (t.flags & NBASR_OPTIM_WEIGHT_NORM) != 0 && c != 0.f};
    const int n = ck.length, tid = threadIdx.x;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
    int done = 0;
    if (vec) {
        const int n4 = n >> 2;
        gfloat4* __restrict__ p4 = (gfloat4*)p;
        const gfloat4* __restrict__ g4 = (const gfloat4*)g;
        gfloat4* __restrict__ m4 = (gfloat4*)m;
        gfloat4* __restrict__ v4 = (gfloat4*)v;
        for (int i = tid; i < n4; i += kThreads) {
            f32x4 pp = p4[i], mm = m4[i], vv = v4[i];
            const f32x4 gg = g4[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pp[e], me = mm[e], ve = vv[e];
                up(pe, gg[e], me, ve);
                pp[e] = pe; mm[e] = me; vv[e] = ve;
            }
            p4[i] = pp; m4[i] = mm; v4[i] = vv;
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += kThreads) {
        float pp = p[i], mm = m[i], vv = v[i];
        up(pp, g[i], mm, vv);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

}  // namespace
}  // namespace nbasr

using namespace nbasr;

extern "C" size_t nbasr_optim_table_bytes(int n_tensors, int n_chunks)
{
    if (n_tensors <= 0 || n_chunks <= 0) return 0;
    return static_cast<size_t>(n_tensors) * sizeof(nbasr_optim_tensor) + static_cast<size_t>(n_chunks) * sizeof(nbasr_optim_chunk);
}

extern "C" size_t nbasr_optim_workspace_bytes(int n_tensors, int n_chunks)
{
    if (n_tensors <= 0 || n_chunks <= 0) return 0;
    // partials[n_chunks][3] doubles | coefs[n_tensors] floats | scale
    return static_cast<size_t>(n_chunks) * 3 * sizeof(double) + (static_cast<size_t>(n_tensors) + 1) * sizeof(float);
}

extern "C" int nbasr_optim_adam_step(const void* table, int n_tensors, int n_chunks, void* workspace, float* total_norm, double beta1,
                                     double beta2, double eps, double max_norm, double weight_norm_coef, nbasr_stream_t stream)
{
    clear_error();
    NBASR_REQUIRE(n_tensors > 0 && n_chunks > 0, NBASR_EINVAL, "nbasr_optim_adam_step: n_tensors=%d and n_chunks=%d must be positive", n_tensors,
                  n_chunks);
    NBASR_REQUIRE(n_chunks >= n_tensors, NBASR_EINVAL, "nbasr_optim_adam_step: n_chunks=%d < n_tensors=%d (every tensor has at least one chunk)",
                  n_chunks, n_tensors);
    NBASR_REQUIRE(table && workspace && total_norm, NBASR_ENULL, "nbasr_optim_adam_step: table, workspace and total_norm must be non-NULL");
    NBASR_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, NBASR_EALIGN,
                  "nbasr_optim_adam_step: table and workspace must be 8-byte aligned");
    NBASR_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, NBASR_EINVAL,
                  "nbasr_optim_adam_step: beta1=%g and beta2=%g must be in [0, 1), eps=%g >= 0", beta1, beta2, eps);
    NBASR_REQUIRE(weight_norm_coef == weight_norm_coef && max_norm == max_norm, NBASR_EINVAL, "nbasr_optim_adam_step: NaN max_norm / weight_norm_coef");
    const nbasr_optim_tensor* tensors = static_cast<const nbasr_optim_tensor*>(table);
    const nbasr_optim_chunk* chunks = reinterpret_cast<const nbasr_optim_chunk*>(tensors + n_tensors);
    double* partials = static_cast<double*>(workspace);
    float* coefs = reinterpret_cast<float*>(partials + 3 * static_cast<size_t>(n_chunks));
    float* scale = coefs + n_tensors;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(optim_reduce_kernel, dim3(n_chunks), dim3(kThreads), 0, s, tensors, chunks, partials);
    hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(kFinalThreads), 0, s, tensors, n_tensors, partials, coefs, scale, total_norm,
                       weight_norm_coef, max_norm);
    hipLaunchKernelGGL(optim_apply_kernel, dim3(n_chunks), dim3(kThreads), 0, s, tensors, chunks, coefs, scale, static_cast<float>(1.0 - beta1),
                       static_cast<float>(beta2), static_cast<float>(1.0 - beta2), static_cast<float>(eps));
    return launch_status("nbasr_optim_adam_step");
}
