// undistort_kernels.hip — cv2.undistortPoints for gfx950: per call (k_undistort_points) and on the resident keypoints
// (k_undistort_frames).  The reference carries the coefficients and never uses them (src/image_and_keypoints.py:21-25).
// OpenCV 4.7's undistort.dispatch.cpp with its default termination, restated from its source as remembered; parity with a cv2
// build is unpinned.  The checker is tests/undistort_reference.py: the same operations in the same order, byte for byte.
#include "vo_internal.h"

// One point.  All arithmetic is f64, left to right, one rounding per operation (-ffp-contract=off):
//   x = (u - cx) (1 / fx), y = (v - cy) (1 / fy); five fixed-point sweeps of the inverse model, left at the first negative
//   icdist with the start values (cv2's fallback outside the model's valid range); then RR (x, y, 1) and the division by its w.
// A NaN compares false with 0, takes every sweep and comes out NaN; nothing here indexes memory by a value.
__device__ __forceinline__ void undistort_one(const UndistortParams& c, double u, double v, double* ox, double* oy)
{
    const double ifx = 1.0 / c.fx, ify = 1.0 / c.fy;
    double x = (u - c.cx) * ifx, y = (v - c.cy) * ify;
    const double x0 = x, y0 = y;
    for (int it = 0; it < 5; it++) {
        const double r2 = x * x + y * y;
        const double icdist = (1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2) / (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
        if (icdist < 0.0) { x = x0; y = y0; break; }
        const double dx = ((2.0 * c.p1) * x) * y + c.p2 * (r2 + (2.0 * x) * x);
        const double dy = c.p1 * (r2 + (2.0 * y) * y) + ((2.0 * c.p2) * x) * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    const double xx = c.RR[0] * x + c.RR[1] * y + c.RR[2];
    const double yy = c.RR[3] * x + c.RR[4] * y + c.RR[5];
    const double ww = 1.0 / (c.RR[6] * x + c.RR[7] * y + c.RR[8]);
    *ox = xx * ww;
    *oy = yy * ww;
}

// One lane per point; the grid tail is guarded.
__global__ __launch_bounds__(256) void k_undistort_points(const void* pts, int point_type, int N, UndistortParams up, void* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double u, v, x, y;
    if (point_type == 0) { u = ((const double*)pts)[2 * (size_t)i]; v = ((const double*)pts)[2 * (size_t)i + 1]; }
    else                 { u = (double)((const float*)pts)[2 * (size_t)i]; v = (double)((const float*)pts)[2 * (size_t)i + 1]; }
    undistort_one(up, u, v, &x, &y);
    if (point_type == 0) { double* o = (double*)out + 2 * (size_t)i; o[0] = x; o[1] = y; }
    else                 { float* o = (float*)out + 2 * (size_t)i; o[0] = (float)x; o[1] = (float)y; }
}

// The resident form: blockIdx.y = slot (relative to the first), one lane per keypoint below the slot's count as the device holds
// it (clamped to the capacity: a count past it names rows the slot does not have).  Writes kp_xy only.
__global__ __launch_bounds__(256) void k_undistort_frames(float* kp_xy, const int* kp_count, int kp_cap, UndistortParams up)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    int n = kp_count[f];
    n = n < 0 ? 0 : (n > kp_cap ? kp_cap : n);
    if (i >= n) return;
    float* p = kp_xy + ((size_t)f * kp_cap + i) * 2;
    double x, y;
    undistort_one(up, (double)p[0], (double)p[1], &x, &y);
    p[0] = (float)x; p[1] = (float)y;
}

void launch_undistort_points(hipStream_t s, const void* pts, int point_type, int N, UndistortParams up, void* out)
{
    if (N <= 0) return;
    hipLaunchKernelGGL(k_undistort_points, dim3((N + 255) / 256), dim3(256), 0, s, pts, point_type, N, up, out);
}

void launch_undistort_frames(hipStream_t s, float* kp_xy, const int* kp_count, int kp_cap, int F, UndistortParams up)
{
    if (F <= 0 || kp_cap <= 0) return;
    // the y axis of a grid holds 65535 blocks
    for (int f0 = 0; f0 < F; f0 += 65535) {
        const int n = F - f0 < 65535 ? F - f0 : 65535;
        hipLaunchKernelGGL(k_undistort_frames, dim3((kp_cap + 255) / 256, n), dim3(256), 0, s, kp_xy + (size_t)f0 * kp_cap * 2, kp_count + f0, kp_cap, up);
    }
}
