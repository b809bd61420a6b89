// detect_rules.hpp — how keypoints are found in an image (dlco_desc_detect*): a multi-scale determinant of the Hessian on
// box filters over an integral image, the Fast-Hessian family whose keypoint sizes the -scale default of 6.25 was chosen
// for.  The rule in integers, stated once for the host, the kernels (kernels_detect.hip) and the CPU test
// (tests/shim/detect_rules_shim.cpp).  Plain C++: no HIP header, no device, no I/O.
//
// This is NOT OpenCV's SURF, which nothing here can run or pin, and no parity with it is claimed.  It is a rule of this
// library: box sums in uint32 modulo 2^32, responses in int64, one parabola per axis in correctly rounded double
// operations, and a total order of the keypoints, so that every keypoint is the same on every machine and the tests
// compare with equality.
//
// Orientation is not part of this rule: every angle it gives is -1, so the describe calls give the same rows with and without
// use_orientation.  orient_rules.hpp assigns angles (dlco_desc_orient, dlco_desc_detect_oriented).
// Out of scope: a 3-D quadratic fit (the refinement is one parabola per axis); a device-keypoint form of
// dlco_desc_describe_keypoints (a keypoint is 16 bytes: the rows go through the host).
//
// Integral image.  S[y][x] = sum of img[v][u] over v < y, u < x: (H+1) x (W+1) entries of uint32 with wrap-around.  The
// inclusive box(x0, y0, x1, y1) = S[y1+1][x1+1] - S[y0][x1+1] - S[y1+1][x0] + S[y0][x0] modulo 2^32 is exact: no box of the
// rule exceeds 255 * 195^2 < 2^32, even where S itself has wrapped.
//
// Scales.  Octave o = 0 .. n_octaves-1 (at most kMaxOctaves), layer i = 0 .. 3 with filter side L = 3 (2^(o+1) (i+1) + 1):
// 9 15 21 27 | 15 27 39 51 | 27 51 75 99 | 51 99 147 195.  Within L: lobe l = L/3, h = (L-1)/2, hw = l-1, hl = (l-1)/2.
//
// Sample grid of an octave.  Step st = 2^o, margin m = (L3 - 1)/2 of its largest layer; columns x_i = m + st i for
// 0 <= i < nx, nx = (W-1-2m)/st + 1 if W-1-2m >= 0 else 0; rows likewise.  Every filter of the octave lies wholly inside
// the image at every grid point: no border is replicated.  An octave with nx < 3 or ny < 3 yields nothing.
//
// Order.  Keypoints are ordered by R descending, then (octave, layer, j, i) ascending: a total order.  A detection
// returns the first min(n_found, max_keypoints) of it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define DETECT_RULES_HD __host__ __device__
#else
#define DETECT_RULES_HD
#endif

namespace detect_rules {

constexpr int kMaxOctaves = 4;
constexpr int kLayers = 4;

DETECT_RULES_HD inline int filter_side(int o, int i) { return 3 * ((2 << o) * (i + 1) + 1); }
DETECT_RULES_HD inline int step(int o) { return 1 << o; }
DETECT_RULES_HD inline int margin(int o) { return (filter_side(o, kLayers - 1) - 1) / 2; }
// grid points of octave o along an axis of `extent` pixels
DETECT_RULES_HD inline int grid_size(int extent, int o)
{
    const int room = extent - 1 - 2 * margin(o);
    return room >= 0 ? room / step(o) + 1 : 0;
}

// S is any object with at(y, x) -> uint32_t: the integral image in ordinary memory, or a staged piece of it
template <typename Src>
DETECT_RULES_HD inline int64_t box(const Src &S, int x0, int y0, int x1, int y1)
{
    const uint32_t v = S.at(y1 + 1, x1 + 1) - S.at(y0, x1 + 1) - S.at(y1 + 1, x0) + S.at(y0, x0);
    return (int64_t)v;
}

// N(D) = sgn(D) ((256 |D| + L^2 / 2) / L^2) by integer division: symmetric in sign, |N| <= 43520
DETECT_RULES_HD inline int64_t normalise(int64_t D, int L)
{
    const int64_t a = D < 0 ? -D : D, q = (int64_t)L * L;
    const int64_t n = (256 * a + q / 2) / q;
    return D < 0 ? -n : n;
}

// the three box differences at pixel (X, Y) for side L; all have zero weight sum
struct Diffs { int64_t Dxx, Dyy, Dxy; };
template <typename Src>
DETECT_RULES_HD inline Diffs diffs(const Src &S, int X, int Y, int L)
{
    const int l = L / 3, h = (L - 1) / 2, hw = l - 1, hl = (l - 1) / 2;
    Diffs d;
    d.Dyy = box(S, X - hw, Y - h, X + hw, Y + h) - 3 * box(S, X - hw, Y - hl, X + hw, Y + hl);
    d.Dxx = box(S, X - h, Y - hw, X + h, Y + hw) - 3 * box(S, X - hl, Y - hw, X + hl, Y + hw);
    d.Dxy = box(S, X + 1, Y - l, X + l, Y - 1) + box(S, X - l, Y + 1, X - 1, Y + l) - box(S, X - l, Y - l, X - 1, Y - 1) -
            box(S, X + 1, Y + 1, X + l, Y + l);
    return d;
}

// R = 100 N(Dxx) N(Dyy) - 81 N(Dxy)^2, |R| < 2^38
template <typename Src>
DETECT_RULES_HD inline int64_t response(const Src &S, int X, int Y, int L)
{
    const Diffs d = diffs(S, X, Y, L);
    const int64_t nxx = normalise(d.Dxx, L), nyy = normalise(d.Dyy, L), nxy = normalise(d.Dxy, L);
    return 100 * nxx * nyy - 81 * nxy * nxy;
}

// Extrema.  Candidates are layers 1 and 2 at grid points 1 <= i <= nx-2, 1 <= j <= ny-2.  A candidate is a keypoint iff
// R >= threshold and it wins against its 26 neighbours (layer +-1, j +-1, i +-1): with R > R_nb against those that precede
// it in the lexicographic order (layer, j, i), with R >= R_nb against those that follow.  A tie between neighbours so
// yields exactly one keypoint, a flat image none (threshold >= 1).  Vol is any object with at(layer, j, i) -> int64_t.
template <typename Vol>
DETECT_RULES_HD inline bool is_keypoint(const Vol &V, int layer, int j, int i, int64_t threshold)
{
    const int64_t R = V.at(layer, j, i);
    if (R < threshold) return false;
    for (int dl = -1; dl <= 1; dl++)
        for (int dj = -1; dj <= 1; dj++)
            for (int di = -1; di <= 1; di++) {
                if (dl == 0 && dj == 0 && di == 0) continue;
                const int64_t nb = V.at(layer + dl, j + dj, i + di);
                const bool precedes = dl < 0 || (dl == 0 && (dj < 0 || (dj == 0 && di < 0)));
                if (precedes ? !(R > nb) : !(R >= nb)) return false;
            }
    return true;
}

// Refinement: one parabola per axis through (Rm, R0, Rp), the only floating point of the rule.  n = Rm - Rp and
// c = Rm - 2 R0 + Rp are exact in int64 and in double; every step below is one correctly rounded IEEE operation (the
// products with st, a power of two, are exact, so a fused multiply-add cannot change a result).  |offset| <= 1/2.
DETECT_RULES_HD inline double offset(int64_t Rm, int64_t R0, int64_t Rp)
{
    const int64_t n = Rm - Rp, c = Rm - 2 * R0 + Rp;
    return c == 0 ? 0.0 : (double)n / (double)(2 * c);
}
// the same in units of a sixth of the layer distance: layers are 6 st pixels of filter side apart
DETECT_RULES_HD inline double offset6(int64_t Rm, int64_t R0, int64_t Rp)
{
    const int64_t n = Rm - Rp, c = Rm - 2 * R0 + Rp;
    return c == 0 ? 0.0 : (double)(3 * n) / (double)c;
}

// a keypoint (x, y, size, -1) with its response and where it was found
struct Keypoint {
    float x, y, size;
    int64_t R;
    int32_t octave, layer, j, i;
};

// position key of a keypoint: ascending in (octave, layer, j, i); j, i < 2^15
DETECT_RULES_HD inline uint64_t position_key(int o, int layer, int j, int i)
{
    return ((uint64_t)(o * 2 + (layer - 1)) << 30) | ((uint64_t)j << 15) | (uint64_t)i;
}

template <typename Vol>
DETECT_RULES_HD inline Keypoint refine(const Vol &V, int o, int layer, int j, int i)
{
    const int st = step(o), m = margin(o);
    const int64_t R0 = V.at(layer, j, i);
    Keypoint k;
    k.x = (float)((double)(m + st * i) + (double)st * offset(V.at(layer, j, i - 1), R0, V.at(layer, j, i + 1)));
    k.y = (float)((double)(m + st * j) + (double)st * offset(V.at(layer, j - 1, i), R0, V.at(layer, j + 1, i)));
    k.size = (float)((double)filter_side(o, layer) + (double)st * offset6(V.at(layer - 1, j, i), R0, V.at(layer + 1, j, i)));
    k.R = R0;
    k.octave = o; k.layer = layer; k.j = j; k.i = i;
    return k;
}

DETECT_RULES_HD inline bool ordered_before(int64_t Ra, uint64_t pos_a, int64_t Rb, uint64_t pos_b)
{
    return Ra != Rb ? Ra > Rb : pos_a < pos_b;
}

// ---- the rule on the host: what the kernels must reproduce ----------------------------------------------------------------
// the integral image of img [H][pitch] into S [(H+1)][(W+1)]
inline void integral_host(const uint8_t *img, int W, int H, int64_t pitch, uint32_t *S)
{
    const size_t sp = (size_t)W + 1;
    for (size_t x = 0; x < sp; x++) S[x] = 0;
    for (int y = 0; y < H; y++) {
        uint32_t row = 0;
        S[(size_t)(y + 1) * sp] = 0;
        for (int x = 0; x < W; x++) {
            row += img[(int64_t)y * pitch + x];
            S[(size_t)(y + 1) * sp + x + 1] = S[(size_t)y * sp + x + 1] + row;
        }
    }
}

struct IntegralSrc {
    const uint32_t *S;
    int64_t pitch;                                          // entries per row
    DETECT_RULES_HD uint32_t at(int y, int x) const { return S[(int64_t)y * pitch + x]; }
};

// the responses of the four layers of octave o on its whole grid: R[layer][j][i]
struct HostVolume {
    int nx = 0, ny = 0;
    std::vector<int64_t> R;
    int64_t at(int layer, int j, int i) const { return R[((size_t)layer * ny + j) * nx + i]; }
};
inline void responses_host(const uint32_t *S, int W, int H, int o, HostVolume &V)
{
    V.nx = grid_size(W, o); V.ny = grid_size(H, o);
    V.R.assign((size_t)kLayers * V.nx * V.ny, 0);
    const IntegralSrc src{S, (int64_t)W + 1};
    const int st = step(o), m = margin(o);
    for (int layer = 0; layer < kLayers; layer++)
        for (int j = 0; j < V.ny; j++)
            for (int i = 0; i < V.nx; i++)
                V.R[((size_t)layer * V.ny + j) * V.nx + i] = response(src, m + st * i, m + st * j, filter_side(o, layer));
}

// every keypoint of the image, in the rule's order
inline void detect_host(const uint32_t *S, int W, int H, int n_octaves, int64_t threshold, std::vector<Keypoint> &out)
{
    out.clear();
    for (int o = 0; o < n_octaves; o++) {
        HostVolume V;
        responses_host(S, W, H, o, V);
        if (V.nx < 3 || V.ny < 3) continue;
        for (int layer = 1; layer <= 2; layer++)
            for (int j = 1; j <= V.ny - 2; j++)
                for (int i = 1; i <= V.nx - 2; i++)
                    if (is_keypoint(V, layer, j, i, threshold)) out.push_back(refine(V, o, layer, j, i));
    }
    std::sort(out.begin(), out.end(), [](const Keypoint &a, const Keypoint &b) {
        return ordered_before(a.R, position_key(a.octave, a.layer, a.j, a.i), b.R, position_key(b.octave, b.layer, b.j, b.i));
    });
}

}  // namespace detect_rules
