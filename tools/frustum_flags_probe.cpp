// Compiled with the REFERENCE's own flags (CMakeLists.txt:10-11,18: -O3 -march=native -std=c++11; on an FMA-capable
// x86-64 host), this translation unit restates the scalar float lines of Frame::isInFrustum (Frame.cc:454-456, :486)
// and of Fuse's projection loop (ORBmatcher.cc:859-870) exactly as the reference writes them, inside loops over the
// points with the early `continue`s, so that GCC makes the contraction decisions it makes for src/Frame.cc and
// src/ORBmatcher.cc.  tools/frustum_flags_check.cpp (built -ffp-contract=off) compares the results with the explicit
// forms k_project_points, orb_project_points_host and tests/frustum_ref.py use.  Test infrastructure
// (tests/test_frustum_pin.py); nothing here is linked into the product or the oracle.
namespace frustum_probe {

struct Camera { float fx, fy, cx, cy, mbf, mnMinX, mnMaxX, mnMinY, mnMaxY; };

// Frame::isInFrustum: out[4 i ..] = u, v, mTrackProjXR, invz; kept[i] = passed the depth and bounds tests
void frame_lines(const Camera& c, int n, const float* Pc, float* out, unsigned char* kept) {
    const float &fx = c.fx, &fy = c.fy, &cx = c.cx, &cy = c.cy, &mbf = c.mbf;
    for (int i = 0; i < n; i++) {
        kept[i] = 0;
        const float& PcX = Pc[3 * i];
        const float& PcY = Pc[3 * i + 1];
        const float& PcZ = Pc[3 * i + 2];

        // Check positive depth
        if (PcZ < 0.0f)
            continue;

        // Project in image and check it is not outside
        const float invz = 1.0f / PcZ;
        const float u = fx * PcX * invz + cx;
        const float v = fy * PcY * invz + cy;

        out[4 * i] = u;
        out[4 * i + 1] = v;
        out[4 * i + 3] = invz;
        if (u < c.mnMinX || u > c.mnMaxX)
            continue;
        if (v < c.mnMinY || v > c.mnMaxY)
            continue;

        out[4 * i + 2] = u - mbf * invz;
        kept[i] = 1;
    }
}

// Fuse: out[4 i ..] = u, v, ur, invz; kept[i] = passed the depth test and IsInImage
void fuse_lines(const Camera& c, int n, const float* p3Dc, float* out, unsigned char* kept) {
    const float &fx = c.fx, &fy = c.fy, &cx = c.cx, &cy = c.cy, &bf = c.mbf;
    for (int i = 0; i < n; i++) {
        kept[i] = 0;
        // Depth must be positive
        if (p3Dc[3 * i + 2] < 0.0f)
            continue;

        const float invz = 1 / p3Dc[3 * i + 2];
        const float x = p3Dc[3 * i] * invz;
        const float y = p3Dc[3 * i + 1] * invz;

        const float u = fx * x + cx;
        const float v = fy * y + cy;

        out[4 * i] = u;
        out[4 * i + 1] = v;
        out[4 * i + 3] = invz;
        // Point must be inside the image
        if (!(u >= c.mnMinX && u < c.mnMaxX && v >= c.mnMinY && v < c.mnMaxY))
            continue;

        const float ur = u - bf * invz;
        out[4 * i + 2] = ur;
        kept[i] = 1;
    }
}

}  // namespace frustum_probe
