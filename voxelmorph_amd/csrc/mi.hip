// Global soft (Parzen-window) mutual information between two images and its gradients (include/vxm_hip.h, "mutual information").
// The reference has the loss on its TensorFlow side only (voxelmorph/tf/losses.py:352-367, a wrapper around a class of another package);
// the definition computed here is this project's restatement of the cited formulation, written out in the header.
//
// No buffer proportional to N x K exists: the soft-bin weights wa[n, :], wb[n, :] live in registers (and, in the forward kernel, one
// 64-voxel tile per wave in LDS) and are recomputed by the backward kernel.
//
//   forward   mi_fwd_kernel     one pass over I, J.  A workgroup owns a contiguous chunk of one sample.  Per 64-voxel tile a wave computes
//                               the two weight rows per voxel (lane = voxel, K exp each, no cross-lane traffic), transposes them through
//                               LDS, and feeds v_mfma_f32_32x32x2_f32 with A[bin a][voxel] / B[voxel][bin b]: the 32 x 32 accumulator IS
//                               the joint histogram partial.  The marginals are summed from the same operands.  One partial per workgroup.
//             mi_reduce_kernel  blocks of 16 partials added in their fixed order in float64, then
//             mi_finish_kernel  one block per sample adds those sums in order, forms pab, pa, pb, MI and the
//                               K x K matrix G = dLoss/dpab with the K-vectors dLoss/dpa, dLoss/dpb (Loss = -MI of the sample).
//             mi_mean_kernel    -mean over the batch (B > 1 only; one block writes it itself when B == 1).
//   backward  mi_bwd_kernel     one pass over I, J; a lane pair (l, l + 32) owns a voxel and 16 bins each -- exactly the bins whose rows of
//                               a 32 x 32 MFMA result land in that lane -- so t = G^T wa (+ dpb) and u = G wb (+ dpa) come out of the
//                               matrix pipe next to the weights they are multiplied with: no LDS, two cross-lane adds per image.
// No floating-point atomics anywhere: every sum has one order, the results repeat bit for bit.
#include "vxm_common.h"
#include <cmath>

#define MI_KMAX 32
#define MI_WAVES 4
#define MI_THREADS (64 * MI_WAVES)
#define MI_TILE 64                                   /* voxels per wave and round (forward) */
#define MI_CHUNK_MIN 2048                            /* voxels per workgroup, at least; a multiple of MI_THREADS */
#define MI_MAX_WG 512                                /* workgroups per sample, at most: the workspace does not grow with N */
#define MI_PART (MI_KMAX * MI_KMAX + 2 * MI_KMAX)    /* floats per partial: joint sums, then the two marginal sums */
#define MI_RED 16                                    /* partials one block of the first reduction stage adds */
#define MI_BWD_TILES 16                              /* 32-voxel tiles per wave (backward) */

typedef float mi_f32x16 __attribute__((ext_vector_type(16)));

struct MiCentres { float c[MI_KMAX]; };

static inline int64_t mi_chunk(int64_t N) {
    int64_t per = (N + MI_MAX_WG - 1) / MI_MAX_WG;
    per = (per + MI_THREADS - 1) / MI_THREADS * MI_THREADS;
    return per < MI_CHUNK_MIN ? MI_CHUNK_MIN : per;
}
static inline int mi_parts(int64_t N) { int64_t c = mi_chunk(N); return (int)((N + c - 1) / c); }
static inline int mi_slices(int64_t N) { return (mi_parts(N) + MI_RED - 1) / MI_RED; }
static inline size_t mi_acc_doubles(int B) { return ((size_t)B + 1) / 2 * 2; }       /* the partials behind stay 16-byte aligned */

__device__ __forceinline__ float mi_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }      /* NaN stays NaN */

/* The K normalised weights of one value, lane = voxel; row k of the tile holds the 64 voxels XOR-swizzled by k (conflict-free both ways). */
__device__ __forceinline__ void mi_soft_bins_to_lds(float x, bool valid, const MiCentres& cen, int K, float alpha2, float lo, float hi,
                                                    float* tile, int lane) {
    const float xc = mi_clamp(x, lo, hi);
    float e[MI_KMAX];
    float dmin = INFINITY;
#pragma unroll
    for (int k = 0; k < MI_KMAX; ++k) {
        if (k < K) {
            const float d = xc - cen.c[k];
            e[k] = d * d;
            dmin = fminf(dmin, e[k]);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MI_KMAX; ++k) {
        if (k < K) {                                 /* the shift by the smallest squared distance keeps the denominator >= 1 */
            e[k] = __builtin_amdgcn_exp2f(-alpha2 * (e[k] - dmin));
            s += e[k];
        } else {
            e[k] = 0.f;                              /* padding bins: exactly zero, no exp */
        }
    }
    const float inv = valid ? 1.0f / s : 0.f;
#pragma unroll
    for (int k = 0; k < MI_KMAX; ++k) tile[k * MI_TILE + (lane ^ k)] = e[k] * inv;
}

__global__ __launch_bounds__(MI_THREADS) void mi_fwd_kernel(const float* __restrict__ I, const float* __restrict__ J, MiCentres cen, int K,
                                                            float alpha2, float lo, float hi, int64_t N, int64_t chunk, int P,
                                                            float* __restrict__ part) {
    __shared__ float sw[MI_WAVES][2][MI_KMAX * MI_TILE];            /* 64 KiB */
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = lane & 31, h = lane >> 5;
    const int p = blockIdx.x, b = blockIdx.y;
    const int64_t begin = (int64_t)p * chunk;
    const int64_t end = begin + chunk < N ? begin + chunk : N;
    const float* Ib = I + (int64_t)b * N;
    const float* Jb = J + (int64_t)b * N;
    float* ta = sw[wave][0];
    float* tb = sw[wave][1];

    /* Summation error matters where many voxels share a value (a constant image, a dark background): repeated equal addends round the same
     * way every time.  So the joint sums run in two chains of 16 steps per tile that are folded into `acc` once per tile, and the marginal
     * sums are compensated (Kahan). */
    mi_f32x16 acc, zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = zero[r] = 0.f;
    float ma = 0.f, mb = 0.f, ea = 0.f, eb = 0.f;

    const int rounds = (int)((end - begin + MI_THREADS - 1) / MI_THREADS);          /* uniform over the workgroup */
    int64_t n = begin + (int64_t)wave * MI_TILE + lane;
    float xa = n < end ? Ib[n] : 0.f, xb = n < end ? Jb[n] : 0.f;
    for (int it = 0; it < rounds; ++it) {
        const bool valid = n < end;
        const float ca = xa, cb = xb;
        n += MI_THREADS;
        if (it + 1 < rounds) {                       /* the next tile's values travel while this one is computed */
            xa = n < end ? Ib[n] : 0.f;
            xb = n < end ? Jb[n] : 0.f;
        }
        mi_soft_bins_to_lds(ca, valid, cen, K, alpha2, lo, hi, ta, lane);
        mi_soft_bins_to_lds(cb, valid, cen, K, alpha2, lo, hi, tb, lane);
        __syncthreads();
        mi_f32x16 c0 = zero, c1 = zero;
#pragma unroll 8
        for (int s = 0; s < 32; ++s) {               /* step s contracts voxels s (lanes 0..31) and 32 + s (lanes 32..63) */
            const int v = s + 32 * h;
            const float a = ta[bin * MI_TILE + (v ^ bin)];
            const float bb = tb[bin * MI_TILE + (v ^ bin)];
            if (s & 1) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, c1, 0, 0, 0);
            else c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, c0, 0, 0, 0);
            const float ya = a - ea, sa = ma + ya;
            ea = (sa - ma) - ya;
            ma = sa;
            const float yb = bb - eb, sb = mb + yb;
            eb = (sb - mb) - yb;
            mb = sb;
        }
        acc += c0 + c1;
        __syncthreads();
    }

    /* one partial per workgroup: the waves' sums added in wave order */
    float* mine = &sw[wave][0][0];
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[(8 * (r >> 2) + 4 * h + (r & 3)) * MI_KMAX + bin] = acc[r];
    mine[MI_KMAX * MI_KMAX + h * MI_KMAX + bin] = ma;
    mine[MI_KMAX * MI_KMAX + 2 * MI_KMAX + h * MI_KMAX + bin] = mb;
    __syncthreads();
    float* out = part + ((int64_t)b * P + p) * MI_PART;
    for (int t = threadIdx.x; t < MI_PART; t += MI_THREADS) {
        float s = 0.f;
        if (t < MI_KMAX * MI_KMAX) {
#pragma unroll
            for (int w = 0; w < MI_WAVES; ++w) s += sw[w][0][t];
        } else {
            const int m = t - MI_KMAX * MI_KMAX, which = m >> 5, k = m & 31;
#pragma unroll
            for (int w = 0; w < MI_WAVES; ++w) {
                const float* q = &sw[w][0][MI_KMAX * MI_KMAX + which * 2 * MI_KMAX];
                s += q[k];
                s += q[MI_KMAX + k];
            }
        }
        out[t] = s;
    }
}

/* First stage of the fixed-order float64 sum: block (s, b) adds partials s * MI_RED .. of sample b, cell by cell (a single block walking
 * over all 512 partials is a chain of 512 dependent memory latencies). */
__global__ __launch_bounds__(MI_THREADS) void mi_reduce_kernel(const float* __restrict__ part, int P, int S, double* __restrict__ red) {
    const int s = blockIdx.x, b = blockIdx.y;
    const int p0 = s * MI_RED, p1 = p0 + MI_RED < P ? p0 + MI_RED : P;
    for (int t = threadIdx.x; t < MI_PART; t += MI_THREADS) {
        double a = 0.0;
#pragma unroll 4
        for (int p = p0; p < p1; ++p) a += (double)part[((int64_t)b * P + p) * MI_PART + t];
        red[((int64_t)b * S + s) * MI_PART + t] = a;
    }
}

/* One block per sample, thread t = (a, b) = (t / 32, t % 32). */
__global__ __launch_bounds__(1024) void mi_finish_kernel(const double* __restrict__ red, int S, int K, int64_t N, float* __restrict__ state,
                                                         double* __restrict__ mi, float* __restrict__ loss) {
    __shared__ double spa[MI_KMAX], spb[MI_KMAX];
    __shared__ double r0[1024], r1[1024], r2[1024];
    const int t = threadIdx.x, a = t >> 5, b = t & 31;
    const double* p0 = red + (int64_t)blockIdx.x * S * MI_PART;
    double s = 0.0;
#pragma unroll 4
    for (int p = 0; p < S; ++p) s += p0[(int64_t)p * MI_PART + t];
    if (t < 2 * MI_KMAX) {
        double m = 0.0;
#pragma unroll 4
        for (int p = 0; p < S; ++p) m += p0[(int64_t)p * MI_PART + MI_KMAX * MI_KMAX + t];
        if (t < MI_KMAX) spa[t] = m / (double)N; else spb[t - MI_KMAX] = m / (double)N;
    }
    __syncthreads();
    const double eps = 1e-7;
    double term = 0.0, g = 0.0, qa = 0.0, qb = 0.0;
    if (a < K && b < K) {
        const double pab = s / (double)N;
        const double papb = spa[a] * spb[b] + eps;
        const double r = pab / papb + eps;
        const double lr = log(r);
        term = pab * lr;
        g = lr + pab / (r * papb);                                   /* dMI/dpab */
        const double c = -pab * pab / (r * papb * papb);             /* dMI/dpapb */
        qa = c * spb[b];
        qb = c * spa[a];
    }
    r0[t] = term;
    r1[t] = qa;
    r2[t] = qb;
    __syncthreads();
    float* st = state + (int64_t)blockIdx.x * MI_PART;
    st[t] = (float)(-g);                                             /* Loss of the sample = -MI */
    if (t < MI_KMAX) {
        double da = 0.0, db = 0.0;
        for (int k = 0; k < MI_KMAX; ++k) {
            da += r1[t * MI_KMAX + k];
            db += r2[k * MI_KMAX + t];
        }
        st[MI_KMAX * MI_KMAX + t] = (float)(-da);
        st[MI_KMAX * MI_KMAX + MI_KMAX + t] = (float)(-db);
    }
    for (int w = 512; w >= 1; w >>= 1) {                             /* a fixed tree */
        if (t < w) r0[t] += r0[t + w];
        __syncthreads();
    }
    if (t == 0) {
        mi[blockIdx.x] = r0[0];
        if (gridDim.x == 1) loss[0] = (float)(-r0[0]);
    }
}

__global__ void mi_mean_kernel(const double* __restrict__ mi, int B, float* __restrict__ loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += mi[b];
        loss[0] = (float)(-s / (double)B);
    }
}

/* The 16 bins of a lane: kb(r) = 8 (r / 4) + 4 h + r % 4, the row of register r of a 32 x 32 MFMA result in half h of the wave. */
struct MiRow {
    float w[16];      /* normalised weights of the lane's bins */
    float d[16];      /* clamped value - centre */
    float m;          /* sum over ALL bins of w * d */
    bool pass;        /* the clamp passes the gradient */
};

__device__ __forceinline__ MiRow mi_soft_bins_row(float x, const float (&cr)[16], int K, int h, float alpha2, float lo, float hi) {
    MiRow o;
    const float xc = mi_clamp(x, lo, hi);
    o.pass = x >= lo && x <= hi;
    float dmin = INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int kb = 8 * (r >> 2) + 4 * h + (r & 3);
        o.d[r] = xc - cr[r];
        o.w[r] = o.d[r] * o.d[r];
        if (kb < K) dmin = fminf(dmin, o.w[r]);
    }
    dmin = fminf(dmin, __shfl_xor(dmin, 32));
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int kb = 8 * (r >> 2) + 4 * h + (r & 3);
        float e = 0.f;                               /* padding bins: exactly zero */
        if (kb < K) e = __builtin_amdgcn_exp2f(-alpha2 * (o.w[r] - dmin));
        o.w[r] = e;
        s += e;
    }
    s += __shfl_xor(s, 32);
    const float inv = 1.0f / s;
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        o.w[r] *= inv;
        m += o.w[r] * o.d[r];
    }
    o.m = m + __shfl_xor(m, 32);
    return o;
}

template <bool GI, bool GJ>
__global__ __launch_bounds__(MI_THREADS) void mi_bwd_kernel(const float* __restrict__ I, const float* __restrict__ J, MiCentres cen, int K,
                                                            float alpha2, float scale_host, float lo, float hi, int64_t N,
                                                            const float* __restrict__ state, const float* __restrict__ gloss,
                                                            float* __restrict__ gI, float* __restrict__ gJ) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const float* st = state + (int64_t)b * MI_PART;
    const float scale = gloss[0] * scale_host;       /* gloss / (N B) * (-2 alpha) */

    float cr[16], AJ[16], AI[16];
    mi_f32x16 tJ0, tI0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k0 = 8 * (r >> 2) + (r & 3);
        const int kb = k0 + 4 * h;
        cr[r] = h ? cen.c[k0 + 4] : cen.c[k0];
        AJ[r] = GJ ? st[kb * MI_KMAX + col] : 0.f;                   /* A[i = b][k = a] = G[a][b] */
        AI[r] = GI ? st[col * MI_KMAX + kb] : 0.f;                   /* A[i = a][k = b] = G[a][b] */
        tJ0[r] = GJ ? st[MI_KMAX * MI_KMAX + MI_KMAX + kb] : 0.f;    /* + dLoss/dpb[b] */
        tI0[r] = GI ? st[MI_KMAX * MI_KMAX + kb] : 0.f;              /* + dLoss/dpa[a] */
    }

    const float* Ib = I + (int64_t)b * N;
    const float* Jb = J + (int64_t)b * N;
    const int64_t first = ((int64_t)blockIdx.x * MI_WAVES + wave) * (MI_BWD_TILES * 32);
    for (int tile = 0; tile < MI_BWD_TILES; ++tile) {
        const int64_t base = first + (int64_t)tile * 32;
        if (base >= N) break;                        /* uniform over the wave */
        const int64_t n = base + col;
        const bool valid = n < N;
        const float xa = valid ? Ib[n] : 0.f, xb = valid ? Jb[n] : 0.f;
        const MiRow ra = mi_soft_bins_row(xa, cr, K, h, alpha2, lo, hi);
        const MiRow rb = mi_soft_bins_row(xb, cr, K, h, alpha2, lo, hi);
        mi_f32x16 tJ = tJ0, tI = tI0;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if (GJ) tJ = __builtin_amdgcn_mfma_f32_32x32x2f32(AJ[s], ra.w[s], tJ, 0, 0, 0);
            if (GI) tI = __builtin_amdgcn_mfma_f32_32x32x2f32(AI[s], rb.w[s], tI, 0, 0, 0);
        }
        if (GJ) {
            float g = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) g += tJ[r] * rb.w[r] * (rb.d[r] - rb.m);
            g += __shfl_xor(g, 32);
            if (valid && h == 0) gJ[(int64_t)b * N + n] = rb.pass ? scale * g : 0.f;
        }
        if (GI) {
            float g = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) g += tI[r] * ra.w[r] * (ra.d[r] - ra.m);
            g += __shfl_xor(g, 32);
            if (valid && h == 0) gI[(int64_t)b * N + n] = ra.pass ? scale * g : 0.f;
        }
    }
}

static int mi_check(const char* who, const float* centres, int K, double alpha, float lo, float hi, int B, int64_t N, MiCentres* cen) {
    VXM_REQUIRE(centres, VXM_ERR_NULL_POINTER, "%s: null pointer", who);
    VXM_REQUIRE(K >= 2 && K <= MI_KMAX, VXM_ERR_UNSUPPORTED, "%s: %d bins, 2 .. %d are implemented", who, K, MI_KMAX);
    VXM_REQUIRE(B >= 1 && B <= 65535 && N >= 1, VXM_ERR_BAD_SHAPE, "%s: B=%d N=%lld", who, B, (long long)N);
    VXM_REQUIRE(alpha > 0.0 && std::isfinite(alpha) && lo <= hi, VXM_ERR_UNSUPPORTED, "%s: alpha=%g clip=[%g, %g]", who, alpha, (double)lo,
                (double)hi);
    for (int k = 0; k < MI_KMAX; ++k) cen->c[k] = k < K ? centres[k] : 0.f;
    for (int k = 0; k < K; ++k)
        VXM_REQUIRE(std::isfinite(centres[k]) && (k == 0 || centres[k] > centres[k - 1]), VXM_ERR_UNSUPPORTED,
                    "%s: bin centres must be finite and strictly increasing", who);
    return VXM_OK;
}

extern "C" {
int64_t vxm_mi_chunk(int64_t N) { return N >= 1 ? mi_chunk(N) : 0; }

size_t vxm_mi_workspace_bytes(int B, int64_t N, int K) {
    if (B < 1 || N < 1 || K < 2 || K > MI_KMAX) return 0;
    return sizeof(double) * (mi_acc_doubles(B) + (size_t)B * mi_slices(N) * MI_PART) + sizeof(float) * (size_t)B * mi_parts(N) * MI_PART;
}

int vxm_mi_fwd(const float* I, const float* J, const float* centres, int K, double alpha, float min_clip, float max_clip, float* loss,
               float* state, void* work, size_t work_bytes, int B, int64_t N, void* stream) {
    MiCentres cen;
    if (int e = mi_check("vxm_mi_fwd", centres, K, alpha, min_clip, max_clip, B, N, &cen)) return e;
    VXM_REQUIRE(I && J && loss && state && work, VXM_ERR_NULL_POINTER, "vxm_mi_fwd: null pointer");
    VXM_REQUIRE(work_bytes >= vxm_mi_workspace_bytes(B, N, K), VXM_ERR_WORKSPACE, "vxm_mi_fwd: workspace of %zu bytes, %zu needed", work_bytes,
                vxm_mi_workspace_bytes(B, N, K));
    const int P = mi_parts(N), S = mi_slices(N);
    double* mi = static_cast<double*>(work);
    double* red = mi + mi_acc_doubles(B);
    float* part = reinterpret_cast<float*>(red + (size_t)B * S * MI_PART);
    const float alpha2 = (float)(alpha * 1.4426950408889634);        /* exp(-alpha x) = exp2(-alpha log2(e) x) */
    hipStream_t s = VXM_STREAM(stream);
    hipLaunchKernelGGL(mi_fwd_kernel, dim3(P, B), dim3(MI_THREADS), 0, s, I, J, cen, K, alpha2, min_clip, max_clip, N, mi_chunk(N), P, part);
    hipLaunchKernelGGL(mi_reduce_kernel, dim3(S, B), dim3(MI_THREADS), 0, s, part, P, S, red);
    hipLaunchKernelGGL(mi_finish_kernel, dim3(B), dim3(1024), 0, s, red, S, K, N, state, mi, loss);
    if (B > 1) hipLaunchKernelGGL(mi_mean_kernel, dim3(1), dim3(64), 0, s, mi, B, loss);
    return vxm_check_launch("vxm_mi_fwd");
}

int vxm_mi_bwd(const float* I, const float* J, const float* centres, int K, double alpha, float min_clip, float max_clip, const float* state,
               const float* gloss, float* gI, float* gJ, int B, int64_t N, void* stream) {
    MiCentres cen;
    if (int e = mi_check("vxm_mi_bwd", centres, K, alpha, min_clip, max_clip, B, N, &cen)) return e;
    VXM_REQUIRE(I && J && state && gloss && (gI || gJ), VXM_ERR_NULL_POINTER, "vxm_mi_bwd: null pointer");
    const float alpha2 = (float)(alpha * 1.4426950408889634);
    const float scale = (float)(-2.0 * alpha / ((double)N * (double)B));
    const int64_t per_block = (int64_t)MI_WAVES * MI_BWD_TILES * 32;
    const dim3 grid((unsigned)((N + per_block - 1) / per_block), B), block(MI_THREADS);
    hipStream_t s = VXM_STREAM(stream);
    if (gI && gJ)
        hipLaunchKernelGGL((mi_bwd_kernel<true, true>), grid, block, 0, s, I, J, cen, K, alpha2, scale, min_clip, max_clip, N, state, gloss, gI, gJ);
    else if (gJ)
        hipLaunchKernelGGL((mi_bwd_kernel<false, true>), grid, block, 0, s, I, J, cen, K, alpha2, scale, min_clip, max_clip, N, state, gloss, gI, gJ);
    else
        hipLaunchKernelGGL((mi_bwd_kernel<true, false>), grid, block, 0, s, I, J, cen, K, alpha2, scale, min_clip, max_clip, N, state, gloss, gI, gJ);
    return vxm_check_launch("vxm_mi_bwd");
}
}
