// The C++ mirror's BoW on ResidentFrame (host/ORBmatcher.{h,cc}): ComputeBoW / BoW against ORBVocabulary::transform,
// and the ResidentFrame overloads of SearchForTriangulation and both SearchByBoW forms against the KeyFrameData
// overloads on the same members.  usage: test_frame_bow_mirror <cases.bin> <vocabulary> <results.bin>
// cases.bin (tests/test_gpu_frame_bow_mirror.py writes it): a triangulation pair, then a SearchByBoW pair, each side as
//   int n | n KeyPoints | n x 32 descriptors | n flags | n uright | FeatureVector (int nnodes, per node: id, count, indices)
// the triangulation pair followed by F12 (9 floats), ex, ey, int nlevels, scaleFactors, levelSigma2; the SearchByBoW
// pair preceded by float nnratio.  results.bin: ints, see main().
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../orb-slam-birdview_amd/host/ORBVocabulary.h"
#include "../../orb-slam-birdview_amd/host/ORBmatcher.h"

using namespace ORB_SLAM2;

struct Reader {
    std::vector<char> buf;
    size_t at = 0;
    template <class T>
    T one() {
        T v;
        std::memcpy(&v, &buf[at], sizeof(T));
        at += sizeof(T);
        return v;
    }
    template <class T>
    std::vector<T> many(size_t n) {
        std::vector<T> v(n);
        if (n) std::memcpy(v.data(), &buf[at], n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

struct Side {
    std::vector<KeyPoint> keys;
    std::vector<uint8_t> desc, mp;
    std::vector<float> ur;
    FeatureVector fv;
    void read(Reader& r) {
        const int n = r.one<int>();
        keys = r.many<KeyPoint>(n);
        desc = r.many<uint8_t>((size_t)n * 32);
        mp = r.many<uint8_t>(n);
        ur = r.many<float>(n);
        const int nnodes = r.one<int>();
        for (int j = 0; j < nnodes; j++) {
            const unsigned id = r.one<unsigned>();
            const int cnt = r.one<int>();
            const std::vector<int> idx = r.many<int>(cnt);
            fv[id] = std::vector<unsigned>(idx.begin(), idx.end());
        }
    }
    KeyFrameData kf() const {
        KeyFrameData k;
        k.n = (int)keys.size();
        k.keys = keys.data();
        k.descriptors = desc.data();
        k.featVec = &fv;
        k.hasMapPoint = mp.data();
        k.uRight = ur.data();
        return k;
    }
    ResidentFrame resident() const {
        ResidentFrame R(keys.data(), (int)keys.size(), desc.data(), ur.data(), 0.f, 640.f, 0.f, 480.f);
        R.SetFeatVec(fv);
        return R;
    }
};

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    Reader r;
    {
        std::ifstream f(argv[1], std::ios::binary);
        r.buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    std::vector<int> out;
    try {
        // --- SearchForTriangulation
        Side a, b;
        a.read(r);
        b.read(r);
        const std::vector<float> F12 = r.many<float>(9);
        const float ex = r.one<float>(), ey = r.one<float>();
        const int nlevels = r.one<int>();
        const std::vector<float> scale = r.many<float>(nlevels), sigma2 = r.many<float>(nlevels);
        ORBmatcher m(0.6f, true);
        KeyFrameData ka = a.kf(), kb = b.kf();
        kb.scaleFactors = scale.data();
        kb.levelSigma2 = sigma2.data();
        kb.nlevels = nlevels;
        ResidentFrame Ra = a.resident(), Rb = b.resident();
        out.push_back(Ra.hasBoW() && Rb.hasBoW());
        for (int only_stereo = 0; only_stereo < 2; only_stereo++) {
            std::vector<std::pair<size_t, size_t> > host;
            m.SearchForTriangulation(ka, kb, F12.data(), ex, ey, host, only_stereo != 0);
            ORBmatcher::ResidentTriangulationNeighbour nb{&Rb, b.mp.data(), scale.data(), sigma2.data(), nlevels, {}, ex, ey};
            std::memcpy(nb.F12, F12.data(), sizeof(nb.F12));
            std::vector<std::vector<std::pair<size_t, size_t> > > res;
            const std::vector<ORBmatcher::ResidentTriangulationNeighbour> nbs(2, nb);
            const int total = m.SearchForTriangulation(Ra, a.mp.data(), nbs, res, only_stereo != 0);
            out.push_back((int)host.size());
            out.push_back(total == 2 * (int)host.size() && res.size() == 2 && res[0] == host && res[1] == host);
            for (size_t i = 0; i < res[0].size(); i++) {
                out.push_back((int)res[0][i].first);
                out.push_back((int)res[0][i].second);
            }
        }
        // --- SearchByBoW, both forms
        const float nnratio = r.one<float>();
        Side c, d;
        c.read(r);
        d.read(r);
        ORBmatcher mb(nnratio, true);
        ResidentFrame Rc = c.resident(), Rd = d.resident();
        KeyFrameData kc = c.kf(), kd = d.kf();
        FrameData fd;
        static_cast<FeatureSet&>(fd) = kd;
        std::vector<int> host, res;
        const int hn = mb.SearchByBoW(kc, fd, host), rn = mb.SearchByBoW(Rc, c.mp.data(), Rd, res);
        out.push_back(hn);
        out.push_back(rn == hn && res == host);
        out.push_back((int)res.size());
        out.insert(out.end(), res.begin(), res.end());
        const int hn2 = mb.SearchByBoW(kc, kd, host), rn2 = mb.SearchByBoW(Rc, c.mp.data(), Rd, d.mp.data(), res);
        out.push_back(hn2);
        out.push_back(rn2 == hn2 && res == host);
        out.push_back((int)res.size());
        out.insert(out.end(), res.begin(), res.end());
        // --- ComputeBoW / BoW against ORBVocabulary::transform, one frame alone and two in one call
        ORBVocabulary voc;
        if (!voc.loadFromBinaryFile(argv[2])) return 3;
        int same = 1;
        std::vector<ResidentFrame*> both{&Rc, &Rd};
        Ra.ComputeBoW(voc.context(), voc.handle(), 2);
        ResidentFrame::ComputeBoW(voc.context(), voc.handle(), both, 2);
        const Side* sides[3] = {&a, &c, &d};
        const ResidentFrame* frames[3] = {&Ra, &Rc, &Rd};
        for (int k = 0; k < 3; k++) {
            DescriptorMat dm;
            dm.create((int)sides[k]->keys.size());
            std::memcpy(dm.buf.data(), sides[k]->desc.data(), dm.buf.size());
            BowVector bv, rbv;
            BowFeatureVector fv;
            FeatureVector rfv;
            voc.transform(dm, bv, fv, 2);
            frames[k]->BoW(voc.handle(), rbv, rfv);
            same = same && bv == rbv && fv == rfv && !fv.empty();
        }
        out.push_back(same);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::ofstream f(argv[3], std::ios::binary);
    f.write((const char*)out.data(), (std::streamsize)(out.size() * sizeof(int)));
    return 0;
}
