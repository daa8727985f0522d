// Compiled with the REFERENCE's own flags (CMakeLists.txt:10-11,18: -O3 -march=native -std=c++11; on an
// FMA-capable x86-64 host), this translation unit restates the reprojection gate of Fuse(KeyFrame*, const
// vector<MapPoint*>&, th) (ORBmatcher.cc:914-938) exactly as the reference writes it, inside a loop over the
// candidates with the stereo / mono branch, so that GCC makes the contraction decisions it makes for
// src/ORBmatcher.cc.  tools/fuse_flags_check.cpp (built -ffp-contract=off) compares the results with the explicit
// forms k_projection_best, orb_project_best_host and tests/kf_projection_ref.py use.  Test infrastructure
// (tests/test_fuse_flags.py); nothing here is linked into the product or the oracle.
namespace fuse_probe {

struct KeyPoint { float x, y; int octave; };

// For each candidate: e2 as the reference computes it and whether the candidate is skipped (`continue`).
void fuse_gate(float u, float v, float ur, int n, const KeyPoint* mvKeysUn, const float* mvuRight,
               const float* mvInvLevelSigma2, float* e2_out, unsigned char* skipped) {
    for (int idx = 0; idx < n; idx++) {
        const KeyPoint& kp = mvKeysUn[idx];
        const int& kpLevel = kp.octave;
        skipped[idx] = 0;
        if (mvuRight[idx] >= 0) {
            // Check reprojection error in stereo
            const float& kpx = kp.x;
            const float& kpy = kp.y;
            const float& kpr = mvuRight[idx];
            const float ex = u - kpx;
            const float ey = v - kpy;
            const float er = ur - kpr;
            const float e2 = ex * ex + ey * ey + er * er;
            e2_out[idx] = e2;

            if (e2 * mvInvLevelSigma2[kpLevel] > 7.8) {
                skipped[idx] = 1;
                continue;
            }
        } else {
            const float& kpx = kp.x;
            const float& kpy = kp.y;
            const float ex = u - kpx;
            const float ey = v - kpy;
            const float e2 = ex * ex + ey * ey;
            e2_out[idx] = e2;

            if (e2 * mvInvLevelSigma2[kpLevel] > 5.99) {
                skipped[idx] = 1;
                continue;
            }
        }
    }
}

}  // namespace fuse_probe
