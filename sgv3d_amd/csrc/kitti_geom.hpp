// The float64 box geometry and the keep rule that the KITTI conversion (result2kitti.hip) and the renderer (render.hip) share.
// Both files are compiled with -ffp-contract=off: every expression here rounds once per operation, on host and device alike.
#pragma once

namespace {

constexpr int kMaxClasses = 64;

struct KittiParams {
    int n, max_det, digits, num_classes;
    double thr, img_w, img_h;
    signed char cls[kMaxClasses];              // class index -> 0 Car, 1 Pedestrian, 2 Cyclist, -1 unmapped
};

__host__ __device__ inline double dot3(const double *m, double a, double b, double c) {
    return (m[0] * a + m[1] * b) + m[2] * c;
}

// Corner k of _box_corners((ex, ey, h), yaw, (x, y, z)) in the lidar frame: the offsets (+-ex/2, +-ey/2, 0 | h) turned by
// the yaw matrix [[c, -s, 0], [s, c, 0], [0, 0, 1]], plus the bottom centre.
__host__ __device__ inline void box_corner(int k, double ex, double ey, double h, double c, double s, double x, double y, double z,
                                           double *p) {
    const double hx = ex / 2, hy = ey / 2;
    const double lx = (k & 2) ? -hx : hx;                       // + + - - + + - -
    const double ly = ((k + 1) & 2) ? -hy : hy;                 // + - - + + - - +
    const double lz = (k & 4) ? h : 0.0;
    p[0] = (c * lx + (-s) * ly) + x;
    p[1] = (s * lx + c * ly) + y;
    p[2] = lz + z;
}

__host__ __device__ inline bool kitti_keep(double score, int label, const KittiParams &P, int *cls) {
    if (!(score > P.thr) || label < 0 || label >= P.num_classes) return false;
    *cls = P.cls[label];
    return *cls >= 0;
}

}  // namespace
