// Evaluation metrics on the device (include/vxm_hip.h, "evaluation metrics"): the integer counts behind the reference's hard Dice
// (voxelmorph/py/utils.py:265-287), the same counts fused with the nearest-neighbour warp of the evaluation protocol
// (scripts/tf/test.py:109-112), and the Jacobian determinant of a displacement field with its folding count (py/utils.py:473-516).
//
// Label counting.  A label map is mostly background and piecewise constant: 64 consecutive voxels of the real scan hold 1.8 distinct
// labels on average.  One LDS atomic per lane would put most of a wave on one address, and one pass per label (the reference's
// formulation) reads the maps L times.  Here every voxel is read once and a wave first agrees on its distinct values: the first pending
// lane's value is broadcast (v_readlane), the lanes holding it -- in all the values a lane carries: four with the 16-byte loads -- are
// counted with ballots + popcounts, the label is looked up ONCE for the wave (binary search over the sorted list in LDS, with the previous
// value's result kept -- runs of one label search nothing) and one lane adds the three counts to the block's u32 counters in LDS.  After
// OVL_ROUNDS distinct values the lanes still pending search and add for themselves.  A block flushes its non-zero counters once with
// 64-bit integer atomics: integer sums, so the result does not depend on the order and two runs agree bit for bit.
//
// Same-address global atomics are what these kernels must be sparing with (measured on the full-size volume: 26 880 blocks adding to the
// two words of `stats` took 330 us where the determinant itself takes 38 us; 1024 blocks flushing 90 counters each made up half of the
// label count's 198 us): the label kernels run at most OVL_MAX_BLOCKS blocks of 1024 threads per batch item, and a Jacobian block marches
// over as many planes as keeps the grid at about JAC_MAX_BLOCKS blocks.
#include "vxm_common.h"
#include "vxm_device.h"

namespace {

constexpr int OVL_THREADS = 1024;
constexpr int OVL_MAX_BLOCKS = 256;          // persistent blocks per batch item (one per CU); beyond that a block takes further grid-stride passes
constexpr int OVL_ROUNDS = 4;                // distinct values a wave agrees on before its lanes go their own way
constexpr int JAC_THREADS = 256;
constexpr int JAC_MAX_BLOCKS = 1024;

// index of u in the strictly increasing list, -1 when absent; `==` semantics: -0.0 finds 0, NaN finds nothing
__device__ __forceinline__ int find_label(const float* lab, int L, float u) {
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lab[mid] < u) lo = mid + 1; else hi = mid;
    }
    return (lo < L && lab[lo] == u) ? lo : -1;
}

struct Tally {
    const float* lab;      // LDS: the L labels
    unsigned* cnt;         // LDS: [L][3] = {a == l and b == l, a == l, b == l}
    int L;
    float cu;              // the wave's last looked-up value and its index
    int ci;
};

__device__ __forceinline__ float wave_value(float v, unsigned long long pending) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)pending) - 1);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// the first pending value of the wave among the K values a lane carries; false when nothing is pending
template <int K>
__device__ __forceinline__ bool next_value(const float (&v)[K], const bool (&pend)[K], float& u) {
    bool found = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long m = __ballot(pend[k]);
        if (!found && m) { u = wave_value(v[k], m); found = true; }
    }
    return found;
}

// K voxel pairs per lane; every lane of the wave must call it (valid = false for a lane without voxels)
template <int K>
__device__ __forceinline__ void tally(Tally& t, const float (&va)[K], const float (&vb)[K], bool valid) {
    bool pa[K], pb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { pa[k] = valid && va[k] == va[k]; pb[k] = valid && vb[k] == vb[k]; }     // a NaN equals no label
    const bool first = (threadIdx.x & 63) == 0;
#pragma unroll 1
    for (int r = 0; r < OVL_ROUNDS; ++r) {                           // the distinct values of a; b is counted along for the same value
        float u;
        if (!next_value<K>(va, pa, u)) break;
        unsigned na = 0, nb = 0, ni = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool ea = pa[k] && va[k] == u, eb = pb[k] && vb[k] == u;
            na += (unsigned)__popcll(__ballot(ea)); nb += (unsigned)__popcll(__ballot(eb)); ni += (unsigned)__popcll(__ballot(ea && eb));
            pa[k] = pa[k] && !ea; pb[k] = pb[k] && !eb;
        }
        if (u != t.cu) { t.ci = find_label(t.lab, t.L, u); t.cu = u; }
        if (first && t.ci >= 0) {
            atomicAdd(&t.cnt[3 * t.ci + 1], na);
            if (nb) atomicAdd(&t.cnt[3 * t.ci + 2], nb);
            if (ni) atomicAdd(&t.cnt[3 * t.ci], ni);
        }
    }
#pragma unroll 1
    for (int r = 0; r < OVL_ROUNDS; ++r) {                           // values of b that no agreed value of a matched
        float u;
        if (!next_value<K>(vb, pb, u)) break;
        unsigned nb = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool eb = pb[k] && vb[k] == u;
            nb += (unsigned)__popcll(__ballot(eb));
            pb[k] = pb[k] && !eb;
        }
        if (u != t.cu) { t.ci = find_label(t.lab, t.L, u); t.cu = u; }
        if (first && t.ci >= 0) atomicAdd(&t.cnt[3 * t.ci + 2], nb);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {                                    // many distinct values in this wave: per-lane search and LDS atomics
        if (pa[k]) {
            const int i = find_label(t.lab, t.L, va[k]);
            if (i >= 0) { atomicAdd(&t.cnt[3 * i + 1], 1u); if (vb[k] == va[k]) atomicAdd(&t.cnt[3 * i], 1u); }
        }
        if (pb[k]) {
            const int i = find_label(t.lab, t.L, vb[k]);
            if (i >= 0) atomicAdd(&t.cnt[3 * i + 2], 1u);
        }
    }
}

__device__ __forceinline__ Tally tally_begin(unsigned char* smem, const float* __restrict__ labels, int L) {
    float* lab = reinterpret_cast<float*>(smem);
    unsigned* cnt = reinterpret_cast<unsigned*>(lab + L);
    for (int i = threadIdx.x; i < L; i += OVL_THREADS) lab[i] = labels[i];
    for (int i = threadIdx.x; i < 3 * L; i += OVL_THREADS) cnt[i] = 0u;
    __syncthreads();
    Tally t;
    t.lab = lab; t.cnt = cnt; t.L = L; t.cu = __int_as_float(0x7fc00000); t.ci = -1;       // NaN: the first value is always looked up
    return t;
}

__device__ __forceinline__ void tally_flush(const Tally& t, unsigned long long* __restrict__ counts) {
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * t.L; i += OVL_THREADS) {
        const unsigned c = t.cnt[i];
        if (c) atomicAdd(&counts[i], (unsigned long long)c);
    }
}

// grid (blocks, B).  Per batch row: 16-byte loads over the part both rows reach aligned, a scalar head and tail around it (the whole
// row when the two rows are misaligned differently).
__global__ void __launch_bounds__(OVL_THREADS) k_label_overlap(const float* __restrict__ a, const float* __restrict__ b,
                                                               const float* __restrict__ labels, int L,
                                                               unsigned long long* __restrict__ counts, long long N) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Tally t = tally_begin(smem, labels, L);
    const float* ar = a + (size_t)blockIdx.y * N;
    const float* br = b + (size_t)blockIdx.y * N;
    const unsigned mis_a = (unsigned)((uintptr_t)ar & 15u), mis_b = (unsigned)((uintptr_t)br & 15u);
    long long head = N, nvec = 0;
    if (mis_a == mis_b) {
        head = (long long)(((16u - mis_a) & 15u) >> 2);
        if (head > N) head = N;
        nvec = (N - head) >> 2;
    }
    const long long tail0 = head + 4 * nvec, nscal = head + (N - tail0);
    const long long stride = (long long)gridDim.x * OVL_THREADS;
    const f32x4* av = reinterpret_cast<const f32x4*>(ar + head);
    const f32x4* bv = reinterpret_cast<const f32x4*>(br + head);
    for (long long base = (long long)blockIdx.x * OVL_THREADS; base < nvec; base += stride) {       // wave-uniform trip count
        const long long i = base + threadIdx.x;
        const bool valid = i < nvec;
        f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f}, y = x;
        if (valid) { x = __builtin_nontemporal_load(av + i); y = __builtin_nontemporal_load(bv + i); }
        const float xa[4] = {x[0], x[1], x[2], x[3]}, ya[4] = {y[0], y[1], y[2], y[3]};
        tally<4>(t, xa, ya, valid);
    }
    for (long long base = (long long)blockIdx.x * OVL_THREADS; base < nscal; base += stride) {
        const long long j = base + threadIdx.x;
        const bool valid = j < nscal;
        const long long idx = j < head ? j : j - head + tail0;
        float x[1] = {0.0f}, y[1] = {0.0f};
        if (valid) { x[0] = ar[idx]; y[0] = br[idx]; }
        tally<1>(t, x, y, valid);
    }
    tally_flush(t, counts + (size_t)blockIdx.y * 3 * L);
}

// grid (blocks, B): the nearest-neighbour branch of k_warp3d_fwd (csrc/warp.hip: same helper, same rounding, same bounds test, an outside
// sample loads 0.0 through the buffer descriptor) with the sampled label counted against fixed[p] instead of being written and read back.
__global__ void __launch_bounds__(OVL_THREADS) k_warp3d_label_overlap(const float* __restrict__ seg, const float* __restrict__ flow,
                                                                      const float* __restrict__ fixed, float* __restrict__ warped,
                                                                      const float* __restrict__ labels, int L,
                                                                      unsigned long long* __restrict__ counts, int D, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Tally t = tally_begin(smem, labels, L);
    const int HW = H * W, V = D * HW, b = blockIdx.y;
    const int V4 = V << 2;
    const __amdgpu_buffer_rsrc_t rf = vxm_rsrc(flow + (size_t)b * 3 * V, 3u * (unsigned)V * 4u);
    const __amdgpu_buffer_rsrc_t rs = vxm_rsrc(seg + (size_t)b * V, (unsigned)V4);
    const float* fx = fixed + (size_t)b * V;
    float* wo = warped ? warped + (size_t)b * V : nullptr;
    const int stride = gridDim.x * OVL_THREADS;
    for (int base = blockIdx.x * OVL_THREADS; base < V; base += stride) {
        const int p = base + threadIdx.x;
        const bool valid = p < V;
        float v[1] = {0.0f}, f[1] = {0.0f};
        if (valid) {
            const int d = p / HW, r = p - d * HW, h = r / W, w = r - h * W;
            const int p4 = p << 2;
            const float z = vxm_src_coord(d, vxm_bload(rf, p4, 0), D), y = vxm_src_coord(h, vxm_bload(rf, p4, V4), H),
                        x = vxm_src_coord(w, vxm_bload(rf, p4, 2 * V4), W);
            const float rz = rintf(z), ry = rintf(y), rx = rintf(x);       // nearbyint: round-half-even
            const bool in = (rz >= 0.0f) & (rz <= (float)(D - 1)) & (ry >= 0.0f) & (ry <= (float)(H - 1)) &
                            (rx >= 0.0f) & (rx <= (float)(W - 1));
            const int idx4 = in ? (((int)rz * H + (int)ry) * W + (int)rx) << 2 : VXM_OOB;      // outside: the load returns 0.0
            v[0] = vxm_bload(rs, idx4, 0);
            f[0] = fx[p];
            if (wo) wo[p] = v[0];
        }
        tally<1>(t, v, f, valid);
    }
    tally_flush(t, counts + (size_t)b * 3 * L);
}

// ---- Jacobian determinant.  One thread per voxel column; the six neighbours of each channel come through the cache (a value leaves HBM
// once: the rows a block shares with its neighbours are in L2 / the memory-side cache when the next block asks).  np.gradient's stencil:
// central difference inside, one-sided on the first and last plane of an axis -- the two voxels a difference reads are chosen by index, so
// no out-of-volume neighbour is ever loaded (and none multiplied by zero): a NaN / Inf displacement reaches exactly the voxels whose
// stencil contains it.  The unit is added AFTER the difference (I + grad disp): in fp32 the difference of displacements keeps the bits
// that grad(disp + grid) loses to the grid coordinate.
struct Diff { int lo, hi; float s; };
__device__ __forceinline__ Diff axis_diff(int i, int n, int step) {
    Diff d;
    const bool l = i > 0, h = i < n - 1;
    d.lo = l ? -step : 0; d.hi = h ? step : 0; d.s = (l && h) ? 0.5f : 1.0f;
    return d;
}
__device__ __forceinline__ float diff_at(const float* __restrict__ f, int p, const Diff& d) {
#pragma clang fp contract(off)
    return (f[p + d.hi] - f[p + d.lo]) * d.s;
}

// wave-uniform running counts {det <= 0, det non-finite}
__device__ __forceinline__ void jac_count(float det, bool valid, unsigned (&n)[2]) {
    n[0] += (unsigned)__popcll(__ballot(valid && det <= 0.0f));
    n[1] += (unsigned)__popcll(__ballot(valid && !(fabsf(det) < __builtin_inff())));
}
// the waves' counts -> one 64-bit atomic each per block
__device__ __forceinline__ void jac_stats(const unsigned (&n)[2], unsigned long long* __restrict__ stats) {
    __shared__ unsigned s_cnt[2][JAC_THREADS / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_cnt[0][wave] = n[0]; s_cnt[1][wave] = n[1]; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned c = 0;
        for (int k = 0; k < JAC_THREADS / 64; ++k) c += s_cnt[threadIdx.x][k];
        if (c) atomicAdd(&stats[threadIdx.x], (unsigned long long)c);
    }
}

// grid (ceil(H W / 256), ceil(D / planes), B): a block marches over `planes` planes of its 256 columns
__global__ void __launch_bounds__(JAC_THREADS) k_jacdet3d(const float* __restrict__ disp, float* __restrict__ det,
                                                          unsigned long long* __restrict__ stats, int D, int H, int W, int planes) {
#pragma clang fp contract(off)
    const int HW = H * W, V = D * HW;
    const int p2 = blockIdx.x * JAC_THREADS + threadIdx.x, b = blockIdx.z;
    const bool valid = p2 < HW;
    const int q = valid ? p2 : 0;                                        // an idle lane follows column 0 and writes nothing
    const int h = q / W, w = q - h * W;
    const Diff dh = axis_diff(h, H, W), dw = axis_diff(w, W, 1);
    const float* f0 = disp + (size_t)b * 3 * V;
    const float* f1 = f0 + V;
    const float* f2 = f1 + V;
    const int d0 = blockIdx.y * planes, d1 = min(d0 + planes, D);
    unsigned n[2] = {0u, 0u};
    for (int d = d0; d < d1; ++d) {
        const int p = d * HW + q;
        const Diff dd = axis_diff(d, D, HW);
        // rows of py/utils.py:500-502: dx = d/d(axis 0), dy = d/d(axis 1), dz = d/d(axis 2) of the three components
        const float dx0 = diff_at(f0, p, dd) + 1.0f, dx1 = diff_at(f1, p, dd), dx2 = diff_at(f2, p, dd);
        const float dy0 = diff_at(f0, p, dh), dy1 = diff_at(f1, p, dh) + 1.0f, dy2 = diff_at(f2, p, dh);
        const float dz0 = diff_at(f0, p, dw), dz1 = diff_at(f1, p, dw), dz2 = diff_at(f2, p, dw) + 1.0f;
        const float j0 = dx0 * (dy1 * dz2 - dy2 * dz1);                  // py/utils.py:505-509
        const float j1 = dx1 * (dy0 * dz2 - dy2 * dz0);
        const float j2 = dx2 * (dy0 * dz1 - dy1 * dz0);
        const float jd = (j0 - j1) + j2;
        if (det && valid) det[(size_t)b * V + p] = jd;
        if (stats) jac_count(jd, valid, n);
    }
    if (stats) jac_stats(n, stats + 2 * b);
}

// grid (blocks, 1, B), grid-stride over the pixels
__global__ void __launch_bounds__(JAC_THREADS) k_jacdet2d(const float* __restrict__ disp, float* __restrict__ det,
                                                          unsigned long long* __restrict__ stats, int H, int W) {
#pragma clang fp contract(off)
    const int V = H * W, b = blockIdx.z;
    const float* f0 = disp + (size_t)b * 2 * V;
    const float* f1 = f0 + V;
    unsigned n[2] = {0u, 0u};
    const int stride = gridDim.x * JAC_THREADS;
    for (int base = blockIdx.x * JAC_THREADS; base < V; base += stride) {
        const int p = base + threadIdx.x;
        const bool valid = p < V;
        float jd = 1.0f;
        if (valid) {
            const int h = p / W, w = p - h * W;
            const Diff dh = axis_diff(h, H, W), dw = axis_diff(w, W, 1);
            const float dx0 = diff_at(f0, p, dh) + 1.0f, dx1 = diff_at(f1, p, dh);
            const float dy0 = diff_at(f0, p, dw), dy1 = diff_at(f1, p, dw) + 1.0f;
            jd = dx0 * dy1 - dy0 * dx1;                                  // py/utils.py:516
            if (det) det[(size_t)b * V + p] = jd;
        }
        if (stats) jac_count(jd, valid, n);
    }
    if (stats) jac_stats(n, stats + 2 * b);
}

int overlap_blocks(long long n, int per_block) {
    long long g = (n + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > OVL_MAX_BLOCKS ? OVL_MAX_BLOCKS : g));
}

// planes a k_jacdet3d block marches over: the fewest that keep the grid of one batch item at JAC_MAX_BLOCKS blocks or below
int jac_planes(int D, int H, int W) {
    const long long bx = ((long long)H * W + JAC_THREADS - 1) / JAC_THREADS;
    const long long planes = (bx * D + JAC_MAX_BLOCKS - 1) / JAC_MAX_BLOCKS;
    return (int)(planes < 1 ? 1 : (planes > D ? D : planes));
}

int check_labels(const char* fn, int L) {
    VXM_REQUIRE(L >= 1 && L <= VXM_LABELS_MAX, VXM_ERR_UNSUPPORTED, "%s: %d labels (1 .. %d)", fn, L, VXM_LABELS_MAX);
    return VXM_OK;
}

bool jac3d_shape_ok(int B, int D, int H, int W) {
    return B >= 1 && B <= 65535 && D >= 2 && H >= 2 && W >= 2 && D <= 65535 && (long long)D * H * W < (1ll << 28);
}

}  // namespace

extern "C" {

int vxm_label_overlap_blocks(int64_t N) { return N < 1 ? 0 : overlap_blocks((long long)N, 4 * OVL_THREADS); }
int vxm_jacdet3d_planes(int D, int H, int W) { return jac3d_shape_ok(1, D, H, W) ? jac_planes(D, H, W) : 0; }

int vxm_label_overlap(const float* a, const float* b, const float* labels_sorted, int L, int64_t* counts, int B, int64_t N, void* stream) {
    if (int e = check_labels("vxm_label_overlap", L)) return e;
    VXM_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && N <= (1ll << 40), VXM_ERR_BAD_SHAPE, "vxm_label_overlap: bad shape B=%d N=%lld", B, (long long)N);
    VXM_REQUIRE(a && b && labels_sorted && counts, VXM_ERR_NULL_POINTER, "vxm_label_overlap: null pointer");
    VXM_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)labels_sorted) & 3u) == 0 && ((uintptr_t)counts & 7u) == 0, VXM_ERR_UNSUPPORTED,
                "vxm_label_overlap: maps must be 4-byte and counts 8-byte aligned");
    if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 3 * (size_t)L * B, VXM_STREAM(stream)) != hipSuccess) return vxm_check_launch("vxm_label_overlap (clear)");
    hipLaunchKernelGGL(k_label_overlap, dim3(overlap_blocks((long long)N, 4 * OVL_THREADS), B), dim3(OVL_THREADS), 16 * (size_t)L, VXM_STREAM(stream),
                       a, b, labels_sorted, L, reinterpret_cast<unsigned long long*>(counts), (long long)N);
    return vxm_check_launch("vxm_label_overlap");
}

int vxm_warp3d_label_overlap(const float* seg, const float* flow, const float* fixed, float* warped, const float* labels_sorted, int L,
                             int64_t* counts, int B, int D, int H, int W, void* stream) {
    if (int e = check_labels("vxm_warp3d_label_overlap", L)) return e;
    VXM_REQUIRE(B >= 1 && B <= 65535 && D > 1 && H > 1 && W > 1 && (long long)D * H * W < (1ll << 28), VXM_ERR_BAD_SHAPE,
                "vxm_warp3d_label_overlap: bad shape B=%d D=%d H=%d W=%d (every extent > 1, fewer than 2^28 voxels, B <= 65535)", B, D, H, W);
    VXM_REQUIRE(seg && flow && fixed && labels_sorted && counts, VXM_ERR_NULL_POINTER, "vxm_warp3d_label_overlap: null pointer");
    if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 3 * (size_t)L * B, VXM_STREAM(stream)) != hipSuccess)
        return vxm_check_launch("vxm_warp3d_label_overlap (clear)");
    hipLaunchKernelGGL(k_warp3d_label_overlap, dim3(overlap_blocks((long long)D * H * W, OVL_THREADS), B), dim3(OVL_THREADS), 16 * (size_t)L,
                       VXM_STREAM(stream), seg, flow, fixed, warped, labels_sorted, L, reinterpret_cast<unsigned long long*>(counts), D, H, W);
    return vxm_check_launch("vxm_warp3d_label_overlap");
}

int vxm_jacdet3d(const float* disp, float* det, int64_t* stats, int B, int D, int H, int W, void* stream) {
    VXM_REQUIRE(jac3d_shape_ok(B, D, H, W), VXM_ERR_BAD_SHAPE,
                "vxm_jacdet3d: bad shape B=%d D=%d H=%d W=%d (every extent >= 2 as np.gradient asks, fewer than 2^28 voxels, B and D <= 65535)",
                B, D, H, W);
    VXM_REQUIRE(disp && (det || stats), VXM_ERR_NULL_POINTER, "vxm_jacdet3d: null pointer (disp, and at least one of det / stats)");
    if (stats && hipMemsetAsync(stats, 0, sizeof(int64_t) * 2 * (size_t)B, VXM_STREAM(stream)) != hipSuccess) return vxm_check_launch("vxm_jacdet3d (clear)");
    const int planes = jac_planes(D, H, W);
    hipLaunchKernelGGL(k_jacdet3d, dim3(vxm_blocks((long long)H * W, JAC_THREADS), (D + planes - 1) / planes, B), dim3(JAC_THREADS), 0,
                       VXM_STREAM(stream), disp, det, reinterpret_cast<unsigned long long*>(stats), D, H, W, planes);
    return vxm_check_launch("vxm_jacdet3d");
}

int vxm_jacdet2d(const float* disp, float* det, int64_t* stats, int B, int H, int W, void* stream) {
    VXM_REQUIRE(B >= 1 && B <= 65535 && H >= 2 && W >= 2 && (long long)H * W < (1ll << 28), VXM_ERR_BAD_SHAPE,
                "vxm_jacdet2d: bad shape B=%d H=%d W=%d (every extent >= 2 as np.gradient asks, fewer than 2^28 pixels, B <= 65535)", B, H, W);
    VXM_REQUIRE(disp && (det || stats), VXM_ERR_NULL_POINTER, "vxm_jacdet2d: null pointer (disp, and at least one of det / stats)");
    if (stats && hipMemsetAsync(stats, 0, sizeof(int64_t) * 2 * (size_t)B, VXM_STREAM(stream)) != hipSuccess) return vxm_check_launch("vxm_jacdet2d (clear)");
    const long long blocks = ((long long)H * W + JAC_THREADS - 1) / JAC_THREADS;
    hipLaunchKernelGGL(k_jacdet2d, dim3((unsigned)(blocks > JAC_MAX_BLOCKS ? JAC_MAX_BLOCKS : blocks), 1, B), dim3(JAC_THREADS), 0, VXM_STREAM(stream),
                       disp, det, reinterpret_cast<unsigned long long*>(stats), H, W);
    return vxm_check_launch("vxm_jacdet2d");
}

}  // extern "C"
