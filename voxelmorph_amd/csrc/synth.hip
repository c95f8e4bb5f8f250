// SynthMorph image synthesis from label maps (include/vxm_hip.h, "image synthesis from label maps"): the four kernels that turn a warped
// label map and a set of random draws into a training image and its one-hot map.  Forward only (generation is data), every random number is
// an input.
//
//   draw      synth_draw_kernel      image = mean[label] + std[label] * noise.  The per-sample table (labels, means, stds) lives in LDS; a lane
//                                    looks its label up by binary search and keeps the last result (a label map is piecewise constant).
//   one-hot   onehot_kernel          one read of the label per voxel, all Lout planes written as 0.0 / 1.0.
//   blur      blur_strided_kernel    axes 0 and 1: the neighbours are whole rows away, every lane reads them straight from memory (16 bytes per
//             blur_row_kernel        lane where W is a multiple of 4); axis 2: a workgroup stages its 256 voxels plus the halo in LDS.
//                                    Three passes x -> out -> work -> out (DESIGN.md 4.14 has the measured times and why this was shipped).
//   finish    finish_minmax_kernel   per-workgroup minimum / maximum of y = clamp(x * exp(log_bias), 0, 255),
//             finish_apply_kernel    every workgroup reduces its sample's partials in one fixed order, recomputes y and writes
//                                    ((y - mn) / (mx - mn)) ^ gamma.
// No floating-point atomics, no allocation, no synchronisation, nothing read on the host.
#include "vxm_common.h"

namespace {

constexpr int SY_THREADS = 256;
constexpr int SY_MAX_BLOCKS = 2048;          // workgroups per sample of the two table kernels (each loads the table once, then strides)
constexpr int FIN_CHUNK_MIN = 1024;          // voxels per workgroup of the finish kernels, at least; a multiple of 4 * SY_THREADS
constexpr int FIN_MAX_WG = 512;              // partials per sample, at most

// index of u in the strictly increasing list, -1 when absent; `==` semantics: -0.0 finds 0, NaN finds nothing
__device__ __forceinline__ int find_label(const float* lab, int L, float u) {
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lab[mid] < u) lo = mid + 1; else hi = mid;
    }
    return (lo < L && lab[lo] == u) ? lo : -1;
}

struct Lookup {                              // a lane's last looked-up value: runs of one label search nothing
    float u;
    int k;
    __device__ __forceinline__ int operator()(const float* lab, int L, float v) {
        if (!(v == u)) { k = find_label(lab, L, v); u = v; }
        return k;
    }
};

__device__ __forceinline__ float draw_one(const float* mean, const float* sd, int k, float z) {
#pragma clang fp contract(off)                       /* a multiply, then an add */
    if (k < 0) return 0.0f;
    const float p = sd[k] * z;
    return mean[k] + p;
}

/* units: nvec quads of four voxels (16-byte accesses), then the V - 4 nvec voxels behind them one by one */
__global__ __launch_bounds__(SY_THREADS) void synth_draw_kernel(const float* __restrict__ labels, const float* __restrict__ sorted,
                                                                const float* __restrict__ means, const float* __restrict__ stds,
                                                                const float* __restrict__ noise, float* __restrict__ image, int L, int64_t V,
                                                                int64_t nvec) {
    extern __shared__ float tab[];                                   /* [3][L]: labels, means, stds */
    float* lab = tab;
    float* mean = tab + L;
    float* sd = tab + 2 * L;
    const int b = blockIdx.y;
    for (int k = threadIdx.x; k < L; k += SY_THREADS) {
        lab[k] = sorted[k];
        mean[k] = means[(int64_t)b * L + k];
        sd[k] = stds[(int64_t)b * L + k];
    }
    __syncthreads();
    const float* lb = labels + (int64_t)b * V;
    const float* nz = noise + (int64_t)b * V;
    float* o = image + (int64_t)b * V;
    Lookup look = {__int_as_float(0x7fc00000), -1};
    const int64_t units = nvec + (V - 4 * nvec);
    for (int64_t t = (int64_t)blockIdx.x * SY_THREADS + threadIdx.x; t < units; t += (int64_t)gridDim.x * SY_THREADS) {
        if (t < nvec) {
            const float4 l = reinterpret_cast<const float4*>(lb)[t], z = reinterpret_cast<const float4*>(nz)[t];
            float4 r;
            r.x = draw_one(mean, sd, look(lab, L, l.x), z.x);
            r.y = draw_one(mean, sd, look(lab, L, l.y), z.y);
            r.z = draw_one(mean, sd, look(lab, L, l.z), z.z);
            r.w = draw_one(mean, sd, look(lab, L, l.w), z.w);
            reinterpret_cast<float4*>(o)[t] = r;
        } else {
            const int64_t j = 4 * nvec + (t - nvec);
            o[j] = draw_one(mean, sd, look(lab, L, lb[j]), nz[j]);
        }
    }
}

__global__ __launch_bounds__(SY_THREADS) void onehot_kernel(const float* __restrict__ labels, const float* __restrict__ sorted,
                                                            const int* __restrict__ out_index, int L, int Lout, float* __restrict__ onehot,
                                                            int64_t V, int64_t nvec) {
    extern __shared__ float tab[];                                   /* [L] labels, then [L] plane indices */
    float* lab = tab;
    int* plane = reinterpret_cast<int*>(tab + L);
    for (int k = threadIdx.x; k < L; k += SY_THREADS) {
        lab[k] = sorted[k];
        plane[k] = out_index[k];
    }
    __syncthreads();
    const int b = blockIdx.y;
    const float* lb = labels + (int64_t)b * V;
    float* o = onehot + (int64_t)b * Lout * V;
    Lookup look = {__int_as_float(0x7fc00000), -1};
    const int64_t units = nvec + (V - 4 * nvec);
    for (int64_t t = (int64_t)blockIdx.x * SY_THREADS + threadIdx.x; t < units; t += (int64_t)gridDim.x * SY_THREADS) {
        if (t < nvec) {
            const float4 l = reinterpret_cast<const float4*>(lb)[t];
            int k;
            k = look(lab, L, l.x); const int p0 = k < 0 ? -1 : plane[k];
            k = look(lab, L, l.y); const int p1 = k < 0 ? -1 : plane[k];
            k = look(lab, L, l.z); const int p2 = k < 0 ? -1 : plane[k];
            k = look(lab, L, l.w); const int p3 = k < 0 ? -1 : plane[k];
            for (int j = 0; j < Lout; ++j) {
                float4 r;
                r.x = p0 == j ? 1.0f : 0.0f;
                r.y = p1 == j ? 1.0f : 0.0f;
                r.z = p2 == j ? 1.0f : 0.0f;
                r.w = p3 == j ? 1.0f : 0.0f;
                reinterpret_cast<float4*>(o + (int64_t)j * V)[t] = r;
            }
        } else {
            const int64_t i = 4 * nvec + (t - nvec);
            const int k = look(lab, L, lb[i]);
            const int p = k < 0 ? -1 : plane[k];
            for (int j = 0; j < Lout; ++j) o[(int64_t)j * V + i] = p == j ? 1.0f : 0.0f;
        }
    }
}

/* One axis of the blur whose neighbours lie `stride` voxels apart (axis 0: stride H W, axis 1: stride W): y[i] = sum_t taps[t] x[i + (t - R)
 * stride] over the taps inside the volume, t ascending from 0.0f, every multiply and add rounded on its own.  VEC = 4: a lane owns four
 * consecutive voxels of one row (W a multiple of 4, aligned bases). */
template <int VEC>
__global__ __launch_bounds__(SY_THREADS) void blur_strided_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                  const float* __restrict__ taps, int axis, int T, int C, unsigned V,
                                                                  unsigned stride, int extent) {
#pragma clang fp contract(off)
    __shared__ float tp[32];
    const int bc = blockIdx.y;
    if ((int)threadIdx.x < T) tp[threadIdx.x] = taps[((int64_t)(bc / C) * 3 + axis) * T + threadIdx.x];
    __syncthreads();
    const unsigned i = (blockIdx.x * SY_THREADS + threadIdx.x) * VEC;
    if (i >= V) return;
    const float* xs = x + (int64_t)bc * V;
    const int R = (T - 1) / 2;
    const int c = (int)((i / stride) % (unsigned)extent);
    const int t0 = R - c > 0 ? R - c : 0;                            /* c + t - R >= 0 */
    const int t1 = extent - 1 - c + R < T - 1 ? extent - 1 - c + R : T - 1;   /* c + t - R <= extent - 1 */
    if (VEC == 4) {
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int t = t0; t <= t1; ++t) {
            const float4 v = *reinterpret_cast<const float4*>(xs + ((int64_t)i + (int64_t)(t - R) * stride));
            const float w = tp[t];
            acc.x = acc.x + w * v.x;
            acc.y = acc.y + w * v.y;
            acc.z = acc.z + w * v.z;
            acc.w = acc.w + w * v.w;
        }
        *reinterpret_cast<float4*>(out + (int64_t)bc * V + i) = acc;
    } else {
        float acc = 0.0f;
        for (int t = t0; t <= t1; ++t) acc = acc + tp[t] * xs[(int64_t)i + (int64_t)(t - R) * stride];
        out[(int64_t)bc * V + i] = acc;
    }
}

/* The last axis: the neighbours of a voxel are its neighbours in memory.  A workgroup stages its 256 consecutive voxels and R more on either
 * side in LDS (zeros outside the sample); a tap is used only where it stays inside the voxel's own row. */
__global__ __launch_bounds__(SY_THREADS) void blur_row_kernel(const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ taps,
                                                              int T, int C, unsigned V, int W) {
#pragma clang fp contract(off)
    __shared__ float tp[32];
    __shared__ float seg[SY_THREADS + 32];
    const int bc = blockIdx.y;
    if ((int)threadIdx.x < T) tp[threadIdx.x] = taps[((int64_t)(bc / C) * 3 + 2) * T + threadIdx.x];
    const float* xs = x + (int64_t)bc * V;
    const int R = (T - 1) / 2;
    const int64_t i0 = (int64_t)blockIdx.x * SY_THREADS;
    for (int j = threadIdx.x; j < SY_THREADS + 2 * R; j += SY_THREADS) {
        const int64_t g = i0 - R + j;
        seg[j] = (g >= 0 && g < (int64_t)V) ? xs[g] : 0.0f;
    }
    __syncthreads();
    const int64_t i = i0 + threadIdx.x;
    if (i >= (int64_t)V) return;
    const int w = (int)((unsigned)i % (unsigned)W);
    const int t0 = R - w > 0 ? R - w : 0;
    const int t1 = W - 1 - w + R < T - 1 ? W - 1 - w + R : T - 1;
    float acc = 0.0f;
    for (int t = t0; t <= t1; ++t) acc = acc + tp[t] * seg[threadIdx.x + t];
    out[(int64_t)bc * V + i] = acc;
}

inline int64_t fin_chunk(int64_t V) {
    int64_t per = (V + FIN_MAX_WG - 1) / FIN_MAX_WG;
    per = (per + 4 * SY_THREADS - 1) / (4 * SY_THREADS) * (4 * SY_THREADS);
    return per < FIN_CHUNK_MIN ? FIN_CHUNK_MIN : per;
}
inline int fin_parts(int64_t V) { const int64_t c = fin_chunk(V); return (int)((V + c - 1) / c); }

template <bool BIAS>
__device__ __forceinline__ float fin_y(float x, float lb) {
#pragma clang fp contract(off)
    float v = x;
    if (BIAS) v = x * expf(lb);
    return fminf(fmaxf(v, 0.0f), 255.0f);
}

/* A workgroup owns voxels [p chunk, min(V, (p + 1) chunk)) of sample b; chunk is a multiple of 4, so with VEC every quad is 16-byte aligned. */
template <bool VEC, bool BIAS>
__global__ __launch_bounds__(SY_THREADS) void finish_minmax_kernel(const float* __restrict__ x, const float* __restrict__ log_bias, unsigned V,
                                                                   unsigned chunk, int P, float* __restrict__ part) {
    __shared__ float rmn[SY_THREADS], rmx[SY_THREADS];
    const int p = blockIdx.x, b = blockIdx.y;
    const unsigned begin = (unsigned)p * chunk;
    const unsigned end = V - begin < chunk ? V : begin + chunk;
    const float* xs = x + (int64_t)b * V;
    const float* ls = BIAS ? log_bias + (int64_t)b * V : nullptr;
    float mn = __int_as_float(0x7f800000), mx = -mn;
    if (VEC) {
        for (unsigned i = begin + 4 * threadIdx.x; i < end; i += 4 * SY_THREADS) {
            const float4 v = *reinterpret_cast<const float4*>(xs + i);
            float4 l = make_float4(0.f, 0.f, 0.f, 0.f);
            if (BIAS) l = *reinterpret_cast<const float4*>(ls + i);
            const float y0 = fin_y<BIAS>(v.x, l.x), y1 = fin_y<BIAS>(v.y, l.y), y2 = fin_y<BIAS>(v.z, l.z), y3 = fin_y<BIAS>(v.w, l.w);
            mn = fminf(fminf(mn, y0), fminf(y1, fminf(y2, y3)));
            mx = fmaxf(fmaxf(mx, y0), fmaxf(y1, fmaxf(y2, y3)));
        }
    } else {
        for (unsigned i = begin + threadIdx.x; i < end; i += SY_THREADS) {
            const float y = fin_y<BIAS>(xs[i], BIAS ? ls[i] : 0.0f);
            mn = fminf(mn, y);
            mx = fmaxf(mx, y);
        }
    }
    rmn[threadIdx.x] = mn;
    rmx[threadIdx.x] = mx;
    __syncthreads();
    for (int s = SY_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
            rmn[threadIdx.x] = fminf(rmn[threadIdx.x], rmn[threadIdx.x + s]);
            rmx[threadIdx.x] = fmaxf(rmx[threadIdx.x], rmx[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[((int64_t)b * P + p) * 2] = rmn[0];
        part[((int64_t)b * P + p) * 2 + 1] = rmx[0];
    }
}

__device__ __forceinline__ float fin_out(float y, float mn, float range, float g, bool flat, bool unit) {
    if (flat) return 0.0f;
    const float q = (y - mn) / range;
    return unit ? q : powf(q, g);
}

template <bool VEC, bool BIAS>
__global__ __launch_bounds__(SY_THREADS) void finish_apply_kernel(const float* __restrict__ x, const float* __restrict__ log_bias,
                                                                  const float* __restrict__ gamma, const float* __restrict__ part, unsigned V,
                                                                  unsigned chunk, int P, float* __restrict__ out) {
    __shared__ float rmn[SY_THREADS], rmx[SY_THREADS];
    const int p = blockIdx.x, b = blockIdx.y;
    float mn = __int_as_float(0x7f800000), mx = -mn;
    for (int q = threadIdx.x; q < P; q += SY_THREADS) {               /* the sample's partials, the same fixed order in every workgroup */
        mn = fminf(mn, part[((int64_t)b * P + q) * 2]);
        mx = fmaxf(mx, part[((int64_t)b * P + q) * 2 + 1]);
    }
    rmn[threadIdx.x] = mn;
    rmx[threadIdx.x] = mx;
    __syncthreads();
    for (int s = SY_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
            rmn[threadIdx.x] = fminf(rmn[threadIdx.x], rmn[threadIdx.x + s]);
            rmx[threadIdx.x] = fmaxf(rmx[threadIdx.x], rmx[threadIdx.x + s]);
        }
        __syncthreads();
    }
    mn = rmn[0];
    mx = rmx[0];
    const float range = mx - mn, g = gamma[b];
    const bool flat = !(mx > mn), unit = g == 1.0f;
    const unsigned begin = (unsigned)p * chunk;
    const unsigned end = V - begin < chunk ? V : begin + chunk;
    const float* xs = x + (int64_t)b * V;
    const float* ls = BIAS ? log_bias + (int64_t)b * V : nullptr;
    float* o = out + (int64_t)b * V;
    if (VEC) {
        for (unsigned i = begin + 4 * threadIdx.x; i < end; i += 4 * SY_THREADS) {
            const float4 v = *reinterpret_cast<const float4*>(xs + i);
            float4 l = make_float4(0.f, 0.f, 0.f, 0.f);
            if (BIAS) l = *reinterpret_cast<const float4*>(ls + i);
            float4 r;
            r.x = fin_out(fin_y<BIAS>(v.x, l.x), mn, range, g, flat, unit);
            r.y = fin_out(fin_y<BIAS>(v.y, l.y), mn, range, g, flat, unit);
            r.z = fin_out(fin_y<BIAS>(v.z, l.z), mn, range, g, flat, unit);
            r.w = fin_out(fin_y<BIAS>(v.w, l.w), mn, range, g, flat, unit);
            *reinterpret_cast<float4*>(o + i) = r;
        }
    } else {
        for (unsigned i = begin + threadIdx.x; i < end; i += SY_THREADS)
            o[i] = fin_out(fin_y<BIAS>(xs[i], BIAS ? ls[i] : 0.0f), mn, range, g, flat, unit);
    }
}

inline bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

inline unsigned table_blocks(int64_t units) {
    const int64_t n = (units + SY_THREADS - 1) / SY_THREADS;
    return (unsigned)(n < SY_MAX_BLOCKS ? n : SY_MAX_BLOCKS);
}

int bv_check(const char* who, int B, int64_t V) {
    VXM_REQUIRE(B >= 1 && B <= 65535 && V >= 1 && V < ((int64_t)1 << 31), VXM_ERR_BAD_SHAPE, "%s: B=%d V=%lld (1 <= B <= 65535, 1 <= V < 2^31)", who,
                B, (long long)V);
    return VXM_OK;
}

bool blur_shape_ok(int T, int B, int C, int D, int H, int W) {
    return T >= 1 && T <= VXM_BLUR_TAPS_MAX && (T & 1) && B >= 1 && C >= 1 && (int64_t)B * C <= 65535 && D >= 1 && H >= 1 && W >= 1 &&
           (int64_t)D * H * W < ((int64_t)1 << 31);
}

template <bool VEC>
void finish_launch(const float* x, const float* log_bias, const float* gamma, float* out, float* part, int B, int64_t V, hipStream_t s) {
    const unsigned chunk = (unsigned)fin_chunk(V);
    const int P = fin_parts(V);
    if (log_bias) {
        hipLaunchKernelGGL((finish_minmax_kernel<VEC, true>), dim3(P, B), dim3(SY_THREADS), 0, s, x, log_bias, (unsigned)V, chunk, P, part);
        hipLaunchKernelGGL((finish_apply_kernel<VEC, true>), dim3(P, B), dim3(SY_THREADS), 0, s, x, log_bias, gamma, part, (unsigned)V, chunk, P, out);
    } else {
        hipLaunchKernelGGL((finish_minmax_kernel<VEC, false>), dim3(P, B), dim3(SY_THREADS), 0, s, x, log_bias, (unsigned)V, chunk, P, part);
        hipLaunchKernelGGL((finish_apply_kernel<VEC, false>), dim3(P, B), dim3(SY_THREADS), 0, s, x, log_bias, gamma, part, (unsigned)V, chunk, P, out);
    }
}

}  // namespace

extern "C" {
int vxm_synth_draw_fwd(const float* labels, const float* labels_sorted, const float* means, const float* stds, const float* noise, float* image,
                       int L, int B, int64_t V, void* stream) {
    if (int e = bv_check("vxm_synth_draw_fwd", B, V)) return e;
    VXM_REQUIRE(L >= 1 && L <= VXM_SYNTH_LABELS_MAX, VXM_ERR_UNSUPPORTED, "vxm_synth_draw_fwd: %d labels, 1 .. %d are implemented", L,
                VXM_SYNTH_LABELS_MAX);
    VXM_REQUIRE(labels && labels_sorted && means && stds && noise && image, VXM_ERR_NULL_POINTER, "vxm_synth_draw_fwd: null pointer");
    const int64_t nvec = (V % 4 == 0 && aligned16(labels, noise, image, image)) ? V / 4 : 0;
    hipLaunchKernelGGL(synth_draw_kernel, dim3(table_blocks(nvec + (V - 4 * nvec)), B), dim3(SY_THREADS), 3 * sizeof(float) * (size_t)L,
                       VXM_STREAM(stream), labels, labels_sorted, means, stds, noise, image, L, V, nvec);
    return vxm_check_launch("vxm_synth_draw_fwd");
}

int vxm_onehot_fwd(const float* labels, const float* labels_sorted, const int* out_index, int L, int Lout, float* onehot, int B, int64_t V,
                   void* stream) {
    if (int e = bv_check("vxm_onehot_fwd", B, V)) return e;
    VXM_REQUIRE(L >= 1 && L <= VXM_SYNTH_LABELS_MAX && Lout >= 1 && Lout <= VXM_ONEHOT_PLANES_MAX, VXM_ERR_UNSUPPORTED,
                "vxm_onehot_fwd: L=%d Lout=%d (1 .. %d labels, 1 .. %d planes are implemented)", L, Lout, VXM_SYNTH_LABELS_MAX, VXM_ONEHOT_PLANES_MAX);
    VXM_REQUIRE(labels && labels_sorted && out_index && onehot, VXM_ERR_NULL_POINTER, "vxm_onehot_fwd: null pointer");
    const int64_t nvec = (V % 4 == 0 && aligned16(labels, onehot, onehot, onehot)) ? V / 4 : 0;
    hipLaunchKernelGGL(onehot_kernel, dim3(table_blocks(nvec + (V - 4 * nvec)), B), dim3(SY_THREADS), 2 * sizeof(float) * (size_t)L,
                       VXM_STREAM(stream), labels, labels_sorted, out_index, L, Lout, onehot, V, nvec);
    return vxm_check_launch("vxm_onehot_fwd");
}

size_t vxm_blur3d_workspace_bytes(int T, int B, int C, int D, int H, int W) {
    if (!blur_shape_ok(T, B, C, D, H, W)) return 0;
    return sizeof(float) * (size_t)B * C * D * H * W;
}

int vxm_blur3d_fwd(const float* x, const float* taps, int T, float* out, void* work, size_t work_bytes, int B, int C, int D, int H, int W,
                   void* stream) {
    VXM_REQUIRE(T >= 1 && T <= VXM_BLUR_TAPS_MAX && (T & 1), VXM_ERR_BAD_SHAPE, "vxm_blur3d_fwd: T=%d (odd, 1 .. %d)", T, VXM_BLUR_TAPS_MAX);
    VXM_REQUIRE(blur_shape_ok(T, B, C, D, H, W), VXM_ERR_BAD_SHAPE, "vxm_blur3d_fwd: B=%d C=%d D=%d H=%d W=%d (B C <= 65535, fewer than 2^31 voxels)",
                B, C, D, H, W);
    VXM_REQUIRE(x && taps && out && work, VXM_ERR_NULL_POINTER, "vxm_blur3d_fwd: null pointer");
    VXM_REQUIRE(out != x && work != (const void*)x && work != (void*)out, VXM_ERR_UNSUPPORTED, "vxm_blur3d_fwd: x, out and work must be three buffers");
    const size_t need = vxm_blur3d_workspace_bytes(T, B, C, D, H, W);
    VXM_REQUIRE(work_bytes >= need, VXM_ERR_WORKSPACE, "vxm_blur3d_fwd: workspace of %zu bytes, %zu needed", work_bytes, need);
    const int64_t V = (int64_t)D * H * W;
    float* mid = static_cast<float*>(work);
    hipStream_t s = VXM_STREAM(stream);
    const bool vec = W % 4 == 0 && aligned16(x, out, mid, mid);
    const dim3 grid_s(vxm_blocks(V, SY_THREADS * (vec ? 4 : 1)), B * C), grid_r(vxm_blocks(V, SY_THREADS), B * C);
    if (vec) {
        hipLaunchKernelGGL(blur_strided_kernel<4>, grid_s, dim3(SY_THREADS), 0, s, x, out, taps, 0, T, C, (unsigned)V, (unsigned)(H * W), D);
        hipLaunchKernelGGL(blur_strided_kernel<4>, grid_s, dim3(SY_THREADS), 0, s, out, mid, taps, 1, T, C, (unsigned)V, (unsigned)W, H);
    } else {
        hipLaunchKernelGGL(blur_strided_kernel<1>, grid_s, dim3(SY_THREADS), 0, s, x, out, taps, 0, T, C, (unsigned)V, (unsigned)(H * W), D);
        hipLaunchKernelGGL(blur_strided_kernel<1>, grid_s, dim3(SY_THREADS), 0, s, out, mid, taps, 1, T, C, (unsigned)V, (unsigned)W, H);
    }
    hipLaunchKernelGGL(blur_row_kernel, grid_r, dim3(SY_THREADS), 0, s, mid, out, taps, T, C, (unsigned)V, W);
    return vxm_check_launch("vxm_blur3d_fwd");
}

size_t vxm_synth_finish_workspace_bytes(int B, int64_t V) {
    if (B < 1 || B > 65535 || V < 1 || V >= ((int64_t)1 << 31)) return 0;
    return sizeof(float) * 2 * (size_t)B * fin_parts(V);
}

int vxm_synth_finish_fwd(const float* x, const float* log_bias, const float* gamma, float* out, void* work, size_t work_bytes, int B, int64_t V,
                         void* stream) {
    if (int e = bv_check("vxm_synth_finish_fwd", B, V)) return e;
    VXM_REQUIRE(x && gamma && out && work, VXM_ERR_NULL_POINTER, "vxm_synth_finish_fwd: null pointer");
    const size_t need = vxm_synth_finish_workspace_bytes(B, V);
    VXM_REQUIRE(work_bytes >= need, VXM_ERR_WORKSPACE, "vxm_synth_finish_fwd: workspace of %zu bytes, %zu needed", work_bytes, need);
    float* part = static_cast<float*>(work);
    if (V % 4 == 0 && aligned16(x, log_bias, out, out))
        finish_launch<true>(x, log_bias, gamma, out, part, B, V, VXM_STREAM(stream));
    else
        finish_launch<false>(x, log_bias, gamma, out, part, B, V, VXM_STREAM(stream));
    return vxm_check_launch("vxm_synth_finish_fwd");
}
}
