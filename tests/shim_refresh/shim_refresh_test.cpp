// shim_refresh_test.cpp -- the shim's plan cache across a nudged track
// (integration/adjust_mmba_core.cpp, Shim::plan_for): marker positions and
// weights are values a cached plan takes anew (mmba_plan_set_marker_values),
// not part of the cache key.
//
// One scene -- an animated camera over 4 frames with its per-frame rotate
// solved, 5 static bundles, no lens -- in three variants:
//   0  as it is
//   1  one marker's x,y at one frame and another observation's weight changed
//   2  the last observation dropped (another obs_frame list: structure)
// Built as libshimrefresh.so (tests/shim_refresh/Makefile);
// tests/test_shim_refresh.py drives the C entries below.
#include <cfloat>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "adjust_mmba_core.h"

using namespace mmba_shim;

namespace {

struct MemReader : SceneReader {
    std::map<std::string, AttrRead> attrs;  // "node.attr"
    int F = 1;

    AttrRead attr(const std::string &node, const std::string &a, bool force) override {
        auto it = attrs.find(node + "." + a);
        if (it == attrs.end()) return AttrRead{};
        AttrRead r = it->second;
        if (force && !r.animated) {  // keyed per frame: one sample per solve frame
            r.animated = true;
            r.frames.assign(F, r.value);
        }
        return r;
    }
    TransformRead transform(const std::string &) override { return TransformRead{}; }
    LensRead lens(const std::string &) override { return LensRead{}; }
    LensRead lens_node(const std::string &) override { return LensRead{}; }

    void stat(const std::string &na, double v) {
        AttrRead r;
        r.exists = true;
        r.value = v;
        attrs[na] = r;
    }
    void anim(const std::string &na, std::vector<double> v) {
        AttrRead r;
        r.exists = true;
        r.animated = true;
        r.value = v[0];
        r.frames = std::move(v);
        attrs[na] = r;
    }
    void trs(const std::string &path, const double t[3]) {
        static const char *n[9] = {"translateX", "translateY", "translateZ", "rotateX", "rotateY",
                                   "rotateZ",    "scaleX",     "scaleY",     "scaleZ"};
        for (int k = 0; k < 9; ++k) stat(path + "." + n[k], k < 3 ? t[k] : k < 6 ? 0.0 : 1.0);
    }
};

struct Scene {
    SolverInputs in;
    MemReader rd;
    Options so;
    std::vector<double> x0;
};

// marker-major, frame-minor: the 5 x 4 marker positions of tests/shim's
// scene 2 (tests/shim/gen_scene2_markers.py), here without its lens
const double kMarkers[20][2] = {
    {-0.23873034935799486, -0.050894781155829634}, {-0.23181865466579299, -0.06415868658293411},
    {-0.22496889641796142, -0.048549320201375472}, {-0.21805635698669693, -0.026341277304751515},
    {-0.12918474157362708, -0.021228432336373618}, {-0.12170790356735069, -0.033055281860840904},
    {-0.11422490874317545, -0.018575519493559296}, {-0.10638882977015819, -8.9621906492073043e-05},
    {-0.044956863564452644, 0.0016716474101909832}, {-0.03722012829822597, -0.0093059329867673009},
    {-0.029069090752251482, 0.0046899590908291615}, {-0.020263446930858117, 0.020251735335200423},
    {0.021639233221250404, 0.019727113220638085},  {0.029532659655347186, 0.0096641178880656296},
    {0.038486605759479368, 0.023090849868926223},  {0.047876170004553104, 0.0363256114043954},
    {0.075032417674294347, 0.034178340970243096},  {0.083717764827209482, 0.024882861684639553},
    {0.092810152575285257, 0.038010888700753316},  {0.10297730975261896, 0.049418792306458313},
};

std::unique_ptr<Scene> make_scene(int variant) {
    auto sc = std::make_unique<Scene>();
    SolverInputs &in = sc->in;
    MemReader &rd = sc->rd;
    const int F = 4, B = 5;
    rd.F = F;
    in.num_frames = F;
    std::vector<double> tx(F), tz(F), rx(F), ry(F), rz(F);
    for (int f = 0; f < F; ++f) {
        tx[f] = 0.1 * f;
        tz[f] = -0.05 * f;
        rx[f] = 1.0 + 0.5 * f;
        ry[f] = -2.0 + 0.3 * f;
        rz[f] = 0.2 * f;
    }
    const double zero3[3] = {0.0, 0.0, 0.0};
    rd.trs("|cam", zero3);
    rd.anim("|cam.translateX", tx);
    rd.stat("|cam.translateY", 1.0);
    rd.anim("|cam.translateZ", tz);
    rd.anim("|cam.rotateX", rx);
    rd.anim("|cam.rotateY", ry);
    rd.anim("|cam.rotateZ", rz);
    const std::string shape = "|cam|camShape";
    rd.stat(shape + ".horizontalFilmAperture", 36.0 / 25.4);
    rd.stat(shape + ".verticalFilmAperture", 24.0 / 25.4);
    rd.stat(shape + ".focalLength", 35.0);
    rd.stat(shape + ".horizontalFilmOffset", 0.0);
    rd.stat(shape + ".verticalFilmOffset", 0.0);
    rd.stat(shape + ".nearClipPlane", 0.1);
    rd.stat(shape + ".farClipPlane", 10000.0);
    rd.stat(shape + ".cameraScale", 1.0);
    in.cameras = {CameraDesc{"|cam", shape, MMBA_FILM_FIT_HORIZONTAL, 2048, 1556}};
    for (int k = 0; k < B; ++k) {
        const std::string b = "|bundle" + std::to_string(k);
        const double bt[3] = {-4.0 + 2.0 * k, 1.0 + 0.5 * k, -20.0 - 3.0 * k};
        rd.trs(b, bt);
        in.bundles.push_back(b);
        in.markers.push_back({0, k});
    }
    for (int k = 0; k < B; ++k)
        for (int f = 0; f < F; ++f) {
            in.errorToMarkerList.push_back({k, f});
            in.markerPosList.push_back({kMarkers[k * F + f][0], kMarkers[k * F + f][1]});
            in.markerWeightList.push_back(1.0);
        }
    if (variant == 1) {  // marker 2 at frame 1 nudged, marker 3's weight at frame 2
        in.markerPosList[2 * F + 1][0] += 2e-3;
        in.markerPosList[2 * F + 1][1] -= 1e-3;
        in.markerWeightList[3 * F + 2] = 0.25;
    }
    if (variant == 2) {
        in.errorToMarkerList.pop_back();
        in.markerPosList.pop_back();
        in.markerWeightList.pop_back();
    }
    const char *rot[3] = {"rotateX", "rotateY", "rotateZ"};
    for (int a = 0; a < 3; ++a) {
        in.attrs.push_back(AttrDesc{"|cam", rot[a], -FLT_MAX, FLT_MAX, 0.0, 1.0});
        for (int f = 0; f < F; ++f) {
            in.paramToAttrList.push_back({a, f});
            sc->x0.push_back(a == 0 ? rx[f] : (a == 1 ? ry[f] : rz[f]));
        }
    }
    sc->so.iterMax = 100;
    return sc;
}

constexpr int kVariants = 3, kShims = 2;
Shim g_shim[kShims];

}  // namespace

extern "C" {

int refresh_num_params(int variant) {
    return variant < 0 || variant >= kVariants ? -1 : (int)make_scene(variant)->x0.size();
}

int refresh_num_errors(int variant) {
    return variant < 0 || variant >= kVariants
               ? -1
               : 2 * (int)make_scene(variant)->in.errorToMarkerList.size();
}

// 1: the plan keys of the two variants are equal, 0: they differ, -1: a
// scene did not map
int refresh_keys_equal(int a, int b) {
    if (a < 0 || a >= kVariants || b < 0 || b >= kVariants) return -1;
    auto sa = make_scene(a), sb = make_scene(b);
    FlatScene fa, fb;
    if (!fa.build(sa->in, sa->rd) || !fb.build(sb->in, sb->rd)) return -1;
    return fa.plan_key(options_of(sa->so)) == fb.plan_key(options_of(sb->so)) ? 1 : 0;
}

// mmba_shim::solve of a variant through shim `which`: the SolveStatus; x [n],
// fvec [m]
int refresh_solve(int which, int variant, double *x_out, double *fvec_out, char *message,
                  int message_len) {
    if (which < 0 || which >= kShims || variant < 0 || variant >= kVariants) return -9;
    auto sc = make_scene(variant);
    const int m = 2 * (int)sc->in.errorToMarkerList.size();
    std::vector<double> x = sc->x0, f(m), eu(m), ed(m / 2);
    Result r;
    std::string msg;
    const SolveStatus st = solve(g_shim[which], sc->in, sc->rd, sc->so, (int)x.size(), m, x.data(),
                                 f.data(), eu.data(), ed.data(), nullptr, &r, &msg);
    if (message && message_len > 0) {
        std::strncpy(message, msg.c_str(), message_len - 1);
        message[message_len - 1] = 0;
    }
    if (st == kSolved) {
        std::memcpy(x_out, x.data(), sizeof(double) * x.size());
        std::memcpy(fvec_out, f.data(), sizeof(double) * f.size());
    }
    return st;
}

int refresh_cached_plans(int which) {
    return which < 0 || which >= kShims ? -1 : (int)g_shim[which].cached_plans();
}

void refresh_release() {
    for (Shim &s : g_shim) s.release();
}

}  // extern "C"
