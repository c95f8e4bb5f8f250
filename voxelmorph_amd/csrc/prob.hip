// The probabilistic velocity field (include/vxm_hip.h, "probabilistic velocity field"): the KL loss of the reference's TensorFlow side
// (voxelmorph/tf/losses.py:247-349) and the reparameterised sample z = mu + exp(ls / 2) eps (voxelmorph/tf/networks.py:230-232), on
// params [B,6,D,H,W]: channels 0..2 the mean mu, channels 3..5 ls = log sigma^2.
//
//   KL forward   kl_fwd_kernel     one pass over the six planes.  A workgroup owns a contiguous chunk of one sample's voxels; a thread forms the
//                                  fp32 terms of its voxels (sigma term and the three forward differences, three channels each) and adds them
//                                  in float64; one partial of four float64 sums per workgroup, added by a fixed tree.
//                kl_finish_kernel  one block adds the partials in a fixed order and evaluates the loss in float64, rounded to fp32 once.
//   KL backward  kl_bwd_kernel     one pass, all six gradient planes: a +-1 stencil per axis on mu, pointwise on ls (exp recomputed).
//   sample       sample_fwd_kernel / sample_bwd_kernel: pointwise, 16 bytes per lane where every row of the batch is 16-byte aligned
//                                  (V a multiple of 4 and aligned bases), element by element otherwise and for the tail.
// No floating-point atomics: every sum has one order, the results repeat bit for bit.
#include "vxm_common.h"
#include <cmath>

#define KL_THREADS 256
#define KL_CHUNK_MIN 1024                            /* voxels per workgroup, at least; a multiple of KL_THREADS */
#define KL_MAX_WG 512                                /* workgroups per sample, at most */

static inline int64_t kl_chunk(int64_t V) {
    int64_t per = (V + KL_MAX_WG - 1) / KL_MAX_WG;
    per = (per + KL_THREADS - 1) / KL_THREADS * KL_THREADS;
    return per < KL_CHUNK_MIN ? KL_CHUNK_MIN : per;
}
static inline int kl_parts(int64_t V) { int64_t c = kl_chunk(V); return (int)((V + c - 1) / c); }

struct KlGeo {
    int D, H, W;
    unsigned HW, V;
};

__device__ __forceinline__ float kl_deg(int d, int h, int w, const KlGeo& g) {
    return (float)((d > 0) + (d < g.D - 1) + (h > 0) + (h < g.H - 1) + (w > 0) + (w < g.W - 1));
}

__global__ __launch_bounds__(KL_THREADS) void kl_fwd_kernel(const float* __restrict__ params, float lam, KlGeo g, unsigned chunk, int P,
                                                            double* __restrict__ part) {
    __shared__ double red[4][KL_THREADS];
    const int p = blockIdx.x, b = blockIdx.y;
    const unsigned begin = (unsigned)p * chunk;
    const unsigned end = begin + chunk < g.V ? begin + chunk : g.V;
    const float* mu = params + (int64_t)b * 6 * g.V;
    const float* ls = mu + (int64_t)3 * g.V;
    double ssig = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (unsigned i = begin + threadIdx.x; i < end; i += KL_THREADS) {
        const int d = (int)(i / g.HW);
        const unsigned r = i - (unsigned)d * g.HW;
        const int h = (int)(r / (unsigned)g.W);
        const int w = (int)(r - (unsigned)h * (unsigned)g.W);
        const float ld = lam * kl_deg(d, h, w, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* m = mu + (int64_t)c * g.V + i;
            const float l = ls[(int64_t)c * g.V + i];
            ssig += (double)(ld * expf(l) - l);
            const float m0 = m[0];
            if (d < g.D - 1) { const float t = m[g.HW] - m0; s0 += (double)(t * t); }
            if (h < g.H - 1) { const float t = m[g.W] - m0; s1 += (double)(t * t); }
            if (w < g.W - 1) { const float t = m[1] - m0; s2 += (double)(t * t); }
        }
    }
    red[0][threadIdx.x] = ssig;
    red[1][threadIdx.x] = s0;
    red[2][threadIdx.x] = s1;
    red[3][threadIdx.x] = s2;
    __syncthreads();
    for (int s = KL_THREADS / 2; s >= 1; s >>= 1) {                  /* a fixed tree */
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) part[((int64_t)b * P + p) * 4 + threadIdx.x] = red[threadIdx.x][0];
}

/* One block: thread t adds partials t, t + KL_THREADS, ... in that order, a fixed tree adds the threads, thread 0 evaluates the loss. */
__global__ __launch_bounds__(KL_THREADS) void kl_finish_kernel(const double* __restrict__ part, int n, double lambda, double n_all, double n0,
                                                               double n1, double n2, float* __restrict__ loss) {
    __shared__ double red[4][KL_THREADS];
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = threadIdx.x; q < n; q += KL_THREADS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += part[(int64_t)q * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int s = KL_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)                       /* the order written, every operation rounded on its own */
        const double sig = red[0][0] / n_all;
        const double prec = (red[1][0] / n0 + red[2][0] / n1) + red[3][0] / n2;
        loss[0] = (float)(1.5 * (sig + lambda * (0.5 / 3) * prec));
    }
}

__global__ __launch_bounds__(KL_THREADS) void kl_bwd_kernel(const float* __restrict__ params, float lam, float c_ls, float c0, float c1, float c2,
                                                            KlGeo g, const float* __restrict__ gloss, float* __restrict__ gparams) {
    const unsigned i = blockIdx.x * KL_THREADS + threadIdx.x;
    if (i >= g.V) return;
    const int b = blockIdx.y;
    const float go = gloss[0];
    const int d = (int)(i / g.HW);
    const unsigned r = i - (unsigned)d * g.HW;
    const int h = (int)(r / (unsigned)g.W);
    const int w = (int)(r - (unsigned)h * (unsigned)g.W);
    const float ld = lam * kl_deg(d, h, w, g);
    const float* mu = params + (int64_t)b * 6 * g.V;
    const float* ls = mu + (int64_t)3 * g.V;
    float* gmu = gparams + (int64_t)b * 6 * g.V;
    float* gls = gmu + (int64_t)3 * g.V;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* m = mu + (int64_t)c * g.V + i;
        const float m0 = m[0];
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        if (d > 0) t0 = m0 - m[-(int64_t)g.HW];
        if (d < g.D - 1) t0 -= m[g.HW] - m0;
        if (h > 0) t1 = m0 - m[-(int64_t)g.W];
        if (h < g.H - 1) t1 -= m[g.W] - m0;
        if (w > 0) t2 = m0 - m[-1];
        if (w < g.W - 1) t2 -= m[1] - m0;
        gmu[(int64_t)c * g.V + i] = go * ((t0 * c0 + t1 * c1) + t2 * c2);
        const float l = ls[(int64_t)c * g.V + i];
        gls[(int64_t)c * g.V + i] = go * ((ld * expf(l) - 1.0f) * c_ls);
    }
}

/* Row b of the batch: n = 3 V values of mu at params + 6 V b, of ls 3 V behind them, of eps / z at 3 V b.  nvec quads of four go through 16-byte
 * accesses (0 when the rows are not all 16-byte aligned), the rest element by element. */
__global__ __launch_bounds__(KL_THREADS) void sample_fwd_kernel(const float* __restrict__ params, const float* __restrict__ eps,
                                                                float* __restrict__ z, int64_t n, int64_t nvec) {
    const int b = blockIdx.y;
    const float* mu = params + (int64_t)b * 2 * n;
    const float* ls = mu + n;
    const float* e = eps + (int64_t)b * n;
    float* o = z + (int64_t)b * n;
    const int64_t t = (int64_t)blockIdx.x * KL_THREADS + threadIdx.x;
    if (t < nvec) {
        const float4 m = reinterpret_cast<const float4*>(mu)[t], l = reinterpret_cast<const float4*>(ls)[t],
                     x = reinterpret_cast<const float4*>(e)[t];
        float4 r;
        r.x = m.x + expf(0.5f * l.x) * x.x;
        r.y = m.y + expf(0.5f * l.y) * x.y;
        r.z = m.z + expf(0.5f * l.z) * x.z;
        r.w = m.w + expf(0.5f * l.w) * x.w;
        reinterpret_cast<float4*>(o)[t] = r;
    } else {
        const int64_t j = 4 * nvec + (t - nvec);
        if (j < n) o[j] = mu[j] + expf(0.5f * ls[j]) * e[j];
    }
}

__global__ __launch_bounds__(KL_THREADS) void sample_bwd_kernel(const float* __restrict__ params, const float* __restrict__ eps,
                                                                const float* __restrict__ gz, float* __restrict__ gparams, int64_t n,
                                                                int64_t nvec) {
    const int b = blockIdx.y;
    const float* ls = params + (int64_t)b * 2 * n + n;
    const float* e = eps + (int64_t)b * n;
    const float* g = gz + (int64_t)b * n;
    float* gmu = gparams + (int64_t)b * 2 * n;
    float* gls = gmu + n;
    const int64_t t = (int64_t)blockIdx.x * KL_THREADS + threadIdx.x;
    if (t < nvec) {
        const float4 l = reinterpret_cast<const float4*>(ls)[t], x = reinterpret_cast<const float4*>(e)[t],
                     q = reinterpret_cast<const float4*>(g)[t];
        float4 r;
        r.x = q.x * (0.5f * expf(0.5f * l.x)) * x.x;
        r.y = q.y * (0.5f * expf(0.5f * l.y)) * x.y;
        r.z = q.z * (0.5f * expf(0.5f * l.z)) * x.z;
        r.w = q.w * (0.5f * expf(0.5f * l.w)) * x.w;
        reinterpret_cast<float4*>(gmu)[t] = q;
        reinterpret_cast<float4*>(gls)[t] = r;
    } else {
        const int64_t j = 4 * nvec + (t - nvec);
        if (j < n) {
            gmu[j] = g[j];
            gls[j] = g[j] * (0.5f * expf(0.5f * ls[j])) * e[j];
        }
    }
}

static int kl_check(const char* who, double lambda, int B, int D, int H, int W) {
    VXM_REQUIRE(B >= 1 && B <= 65535 && D >= 2 && H >= 2 && W >= 2, VXM_ERR_BAD_SHAPE,
                "%s: B=%d D=%d H=%d W=%d (every extent of the grid must be at least 2: the mean over an empty slice is NaN)", who, B, D, H, W);
    VXM_REQUIRE((int64_t)D * H * W < ((int64_t)1 << 31), VXM_ERR_BAD_SHAPE, "%s: %lld voxels per sample, fewer than 2^31 are implemented", who,
                (long long)((int64_t)D * H * W));
    VXM_REQUIRE(std::isfinite(lambda), VXM_ERR_UNSUPPORTED, "%s: prior_lambda=%g", who, lambda);
    return VXM_OK;
}

static inline bool sample_vec_ok(int64_t V, const void* a, const void* b, const void* c, const void* d) {
    return V % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
                           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

extern "C" {
size_t vxm_kl_workspace_bytes(int B, int D, int H, int W) {
    if (B < 1 || B > 65535 || D < 2 || H < 2 || W < 2 || (int64_t)D * H * W >= ((int64_t)1 << 31)) return 0;
    return sizeof(double) * 4 * (size_t)B * kl_parts((int64_t)D * H * W);
}

int vxm_kl_fwd(const float* params, double prior_lambda, float* loss, void* work, size_t work_bytes, int B, int D, int H, int W, void* stream) {
    if (int e = kl_check("vxm_kl_fwd", prior_lambda, B, D, H, W)) return e;
    VXM_REQUIRE(params && loss && work, VXM_ERR_NULL_POINTER, "vxm_kl_fwd: null pointer");
    VXM_REQUIRE(work_bytes >= vxm_kl_workspace_bytes(B, D, H, W), VXM_ERR_WORKSPACE, "vxm_kl_fwd: workspace of %zu bytes, %zu needed", work_bytes,
                vxm_kl_workspace_bytes(B, D, H, W));
    const int64_t V = (int64_t)D * H * W;
    const KlGeo g = {D, H, W, (unsigned)(H * W), (unsigned)V};
    const int P = kl_parts(V);
    double* part = static_cast<double*>(work);
    const double rows = 3.0 * (double)B;                             /* N_a = 3 B (V / S_a) (S_a - 1), an integer */
    hipStream_t s = VXM_STREAM(stream);
    hipLaunchKernelGGL(kl_fwd_kernel, dim3(P, B), dim3(KL_THREADS), 0, s, params, (float)prior_lambda, g, (unsigned)kl_chunk(V), P, part);
    hipLaunchKernelGGL(kl_finish_kernel, dim3(1), dim3(KL_THREADS), 0, s, part, B * P, prior_lambda, rows * (double)V,
                       rows * (double)(V / D * (D - 1)), rows * (double)(V / H * (H - 1)), rows * (double)(V / W * (W - 1)), loss);
    return vxm_check_launch("vxm_kl_fwd");
}

int vxm_kl_bwd(const float* params, double prior_lambda, const float* gloss, float* gparams, int B, int D, int H, int W, void* stream) {
    if (int e = kl_check("vxm_kl_bwd", prior_lambda, B, D, H, W)) return e;
    VXM_REQUIRE(params && gloss && gparams, VXM_ERR_NULL_POINTER, "vxm_kl_bwd: null pointer");
    const int64_t V = (int64_t)D * H * W;
    const KlGeo g = {D, H, W, (unsigned)(H * W), (unsigned)V};
    const double rows = 3.0 * (double)B;
    const float c_ls = (float)(1.0 / (2.0 * (double)B * (double)V));
    const float c0 = (float)(0.5 * prior_lambda / (rows * (double)(V / D * (D - 1))));
    const float c1 = (float)(0.5 * prior_lambda / (rows * (double)(V / H * (H - 1))));
    const float c2 = (float)(0.5 * prior_lambda / (rows * (double)(V / W * (W - 1))));
    hipLaunchKernelGGL(kl_bwd_kernel, dim3(vxm_blocks(V, KL_THREADS), B), dim3(KL_THREADS), 0, VXM_STREAM(stream), params, (float)prior_lambda,
                       c_ls, c0, c1, c2, g, gloss, gparams);
    return vxm_check_launch("vxm_kl_bwd");
}

int vxm_sample_logvar_fwd(const float* params, const float* eps, float* z, int B, int64_t V, void* stream) {
    VXM_REQUIRE(B >= 1 && B <= 65535 && V >= 1 && V < ((int64_t)1 << 31), VXM_ERR_BAD_SHAPE, "vxm_sample_logvar_fwd: B=%d V=%lld", B, (long long)V);
    VXM_REQUIRE(params && eps && z, VXM_ERR_NULL_POINTER, "vxm_sample_logvar_fwd: null pointer");
    const int64_t n = 3 * V, nvec = sample_vec_ok(V, params, eps, z, z) ? n / 4 : 0;
    hipLaunchKernelGGL(sample_fwd_kernel, dim3(vxm_blocks(nvec + (n - 4 * nvec), KL_THREADS), B), dim3(KL_THREADS), 0, VXM_STREAM(stream), params,
                       eps, z, n, nvec);
    return vxm_check_launch("vxm_sample_logvar_fwd");
}

int vxm_sample_logvar_bwd(const float* params, const float* eps, const float* gz, float* gparams, int B, int64_t V, void* stream) {
    VXM_REQUIRE(B >= 1 && B <= 65535 && V >= 1 && V < ((int64_t)1 << 31), VXM_ERR_BAD_SHAPE, "vxm_sample_logvar_bwd: B=%d V=%lld", B, (long long)V);
    VXM_REQUIRE(params && eps && gz && gparams, VXM_ERR_NULL_POINTER, "vxm_sample_logvar_bwd: null pointer");
    const int64_t n = 3 * V, nvec = sample_vec_ok(V, params, eps, gz, gparams) ? n / 4 : 0;
    hipLaunchKernelGGL(sample_bwd_kernel, dim3(vxm_blocks(nvec + (n - 4 * nvec), KL_THREADS), B), dim3(KL_THREADS), 0, VXM_STREAM(stream), params,
                       eps, gz, gparams, n, nvec);
    return vxm_check_launch("vxm_sample_logvar_bwd");
}
}
