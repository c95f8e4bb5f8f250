// Affine transforms on the device for gfx950: a matrix as a dense displacement field, optionally right-composed with a dense field.
// HBM-bound; one thread per voxel of the OUTPUT grid, the 64 lanes of a wave walk W; the matrix is 12 wave-uniform floats per sample.
//
// Reference semantics restated (paths relative to the reference root; TensorFlow side, no bit parity claimed):
//   voxelmorph/tf/utils/utils.py:638-699   affine_to_dense_shift (shift_center, warp_right)
//   voxelmorph/tf/utils/utils.py:253-318   compose (matrix left of dense: this kernel with warp_right)
// Coordinate chain (include/vxm_hip.h), fp32, every operation rounded on its own:
//   q[k] = float(i[k]) - c[k]   (+ w[b,k,i] when a right-composed field is given)
//   x[a] = (((M[a,0] q[0]) + (M[a,1] q[1])) + (M[a,2] q[2])) + M[a,3];   shift[b,a,i] = x[a] - (float(i[a]) - c[a])
#include "vxm_common.h"
#include "vxm_device.h"

namespace {

constexpr int AF_T = 256;                    // threads per block: 4 waves along H W of one output plane
constexpr int AF_NV = 12;                    // entries of a 3 x 4 matrix

// affine -> dense shift; the matrix of sample b is M[Bm == 1 ? 0 : b]
__global__ void __launch_bounds__(AF_T) k_affine_shift3d_fwd(const float* __restrict__ mat, int Bm, const float* __restrict__ flow,
                                                             float* __restrict__ shift, int D, int H, int W, int shift_center) {
#pragma clang fp contract(off)
    const int HW = H * W, V = D * HW;
    const int p2 = blockIdx.x * AF_T + threadIdx.x;
    if (p2 >= HW) return;
    const int d = blockIdx.y, b = blockIdx.z;
    const int h = p2 / W, w = p2 - h * W;
    const int p4 = (d * HW + p2) << 2, V4 = V << 2;
    const float* m = mat + (Bm == 1 ? 0 : (size_t)b * AF_NV);
    // 0.5 (S - 1) is exact in fp32 for every extent the entry points accept
    const float c0 = shift_center ? 0.5f * (float)(D - 1) : 0.0f, c1 = shift_center ? 0.5f * (float)(H - 1) : 0.0f,
                c2 = shift_center ? 0.5f * (float)(W - 1) : 0.0f;
    const float g[3] = {(float)d - c0, (float)h - c1, (float)w - c2};           // the grid point about the centre
    float q[3] = {g[0], g[1], g[2]};
    if (flow) {
        const __amdgpu_buffer_rsrc_t rf = vxm_rsrc(flow + (size_t)b * 3 * V, 3u * (unsigned)V * 4u);
        q[0] = q[0] + vxm_bload(rf, p4, 0); q[1] = q[1] + vxm_bload(rf, p4, V4); q[2] = q[2] + vxm_bload(rf, p4, 2 * V4);
    }
    const __amdgpu_buffer_rsrc_t ro = vxm_rsrc(shift + (size_t)b * 3 * V, 3u * (unsigned)V * 4u);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = (((m[4 * a] * q[0]) + (m[4 * a + 1] * q[1])) + (m[4 * a + 2] * q[2])) + m[4 * a + 3];
        vxm_bstore(x - g[a], ro, p4, a * V4);
    }
}

// backward of the shift with respect to the right-composed field: gw[b,k,i] = ((M[0,k] g[0]) + (M[1,k] g[1])) + (M[2,k] g[2]), g = gout[b,:,i]
__global__ void __launch_bounds__(AF_T) k_affine_shift3d_bwd(const float* __restrict__ mat, int Bm, const float* __restrict__ gout,
                                                             float* __restrict__ gflow, int D, int H, int W) {
#pragma clang fp contract(off)
    const int HW = H * W, V = D * HW;
    const int p2 = blockIdx.x * AF_T + threadIdx.x;
    if (p2 >= HW) return;
    const int d = blockIdx.y, b = blockIdx.z;
    const int p4 = (d * HW + p2) << 2, V4 = V << 2;
    const float* m = mat + (Bm == 1 ? 0 : (size_t)b * AF_NV);
    const __amdgpu_buffer_rsrc_t rgo = vxm_rsrc(gout + (size_t)b * 3 * V, 3u * (unsigned)V * 4u);
    const __amdgpu_buffer_rsrc_t rg = vxm_rsrc(gflow + (size_t)b * 3 * V, 3u * (unsigned)V * 4u);
    const float g[3] = {vxm_bload(rgo, p4, 0), vxm_bload(rgo, p4, V4), vxm_bload(rgo, p4, 2 * V4)};
#pragma unroll
    for (int k = 0; k < 3; ++k) vxm_bstore(((m[k] * g[0]) + (m[4 + k] * g[1])) + (m[8 + k] * g[2]), rg, p4, k * V4);
}

int af_check(const char* fn, int Bm, int B, int D, int H, int W) {
    VXM_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, VXM_ERR_BAD_SHAPE, "%s: bad shape B=%d grid %dx%dx%d", fn, B, D, H, W);
    VXM_REQUIRE(Bm == 1 || Bm == B, VXM_ERR_BAD_SHAPE, "%s: %d matrices for a batch of %d (one per sample, or one for all)", fn, Bm, B);
    VXM_REQUIRE((long long)D * H * W < (1ll << 28) && B <= 65535 && D <= 65535, VXM_ERR_BAD_SHAPE,
                "%s: 32-bit byte offsets within the 3 planes of a sample: fewer than 2^28 voxels, B and D <= 65535", fn);
    return VXM_OK;
}

}  // namespace

extern "C" {

int vxm_affine_shift3d_fwd(const float* mat, int Bm, const float* flow, float* shift, int B, int D, int H, int W, int shift_center, void* stream) {
    if (int e = af_check("vxm_affine_shift3d_fwd", Bm, B, D, H, W)) return e;
    VXM_REQUIRE(shift_center == 0 || shift_center == 1, VXM_ERR_UNSUPPORTED, "vxm_affine_shift3d_fwd: shift_center %d (0 or 1)", shift_center);
    VXM_REQUIRE(mat && shift, VXM_ERR_NULL_POINTER, "vxm_affine_shift3d_fwd: null pointer");
    const dim3 grid(vxm_blocks((long long)H * W, AF_T), D, B);
    hipLaunchKernelGGL(k_affine_shift3d_fwd, grid, dim3(AF_T), 0, VXM_STREAM(stream), mat, Bm, flow, shift, D, H, W, shift_center);
    return vxm_check_launch("vxm_affine_shift3d_fwd");
}

int vxm_affine_shift3d_bwd(const float* mat, int Bm, const float* gout, float* gflow, int B, int D, int H, int W, void* stream) {
    if (int e = af_check("vxm_affine_shift3d_bwd", Bm, B, D, H, W)) return e;
    VXM_REQUIRE(mat && gout && gflow, VXM_ERR_NULL_POINTER, "vxm_affine_shift3d_bwd: null pointer");
    const dim3 grid(vxm_blocks((long long)H * W, AF_T), D, B);
    hipLaunchKernelGGL(k_affine_shift3d_bwd, grid, dim3(AF_T), 0, VXM_STREAM(stream), mat, Bm, gout, gflow, D, H, W);
    return vxm_check_launch("vxm_affine_shift3d_bwd");
}

}  // extern "C"
