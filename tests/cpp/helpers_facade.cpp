// helpers_facade.cpp -- the static helpers of the facade's Line3D (include/line3dpp/line3D.h): rotationFromRPY,
// rotationFromQ and decomposeProjectionMatrix, with plain matrix types that have what Eigen's have: (r, c), rows(), cols().
// stdin: n, then n projection matrices (12 doubles, row-major); m, then m lines `roll pitch yaw qw qx qy qz`.
// stdout: per matrix K (9), R (9), t (3); per line rotationFromRPY (9), rotationFromQ (9); doubles with 17 digits.
// Host code only: no device is touched.  Built and run by tests/test_front_ends_more.py.
#include <cstdio>
#include <vector>

#include "line3dpp/line3D.h"

struct Mat {
    int r, c;
    std::vector<double> a;
    Mat(int r_ = 3, int c_ = 3) : r(r_), c(c_), a((size_t)r_ * c_, 0.0) {}
    double& operator()(int i, int j) { return a[(size_t)i * c + j]; }
    double operator()(int i, int j) const { return a[(size_t)i * c + j]; }
    int rows() const { return r; }
    int cols() const { return c; }
};
struct Vec {
    double a[3] = {0, 0, 0};
    double& operator()(int i) { return a[i]; }
    double operator()(int i) const { return a[i]; }
};

static void print9(const Mat& M) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) std::printf("%.17g ", M(i, j));
}

int main() {
    using L3DPP_HIP::Line3D;
    int n = 0;
    if (std::scanf("%d", &n) != 1) return 2;
    for (int k = 0; k < n; ++k) {
        Mat P(3, 4), K, R;
        Vec t;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j)
                if (std::scanf("%lf", &P(i, j)) != 1) return 2;
        Line3D::decomposeProjectionMatrix(P, K, R, t);
        print9(K); print9(R);
        std::printf("%.17g %.17g %.17g\n", t(0), t(1), t(2));
    }
    int m = 0;
    if (std::scanf("%d", &m) != 1) return 2;
    for (int k = 0; k < m; ++k) {
        double v[7];
        for (double& x : v)
            if (std::scanf("%lf", &x) != 1) return 2;
        print9(Line3D::rotationFromRPY<Mat>(v[0], v[1], v[2]));
        print9(Line3D::rotationFromQ<Mat>(v[3], v[4], v[5], v[6]));
        std::printf("\n");
    }
    std::fflush(stdout);
    // neither 3 rows nor 4 columns: reported, outputs untouched
    Mat bad(4, 3), K, R;
    Vec t;
    K(0, 0) = 7.0;
    Line3D::decomposeProjectionMatrix(bad, K, R, t);
    return K(0, 0) == 7.0 ? 0 : 3;
}
