// gtf_extract.hip -- track-candidate extraction on the GPU:
// src/extract/extract_track_candidates.py main (:349-467) after the hot path.
//
//  1. CCA (:332-346): connected components over the ACTIVATED edges of each subgraph
//     (undirected), by min-label hooking + pointer jumping; a subgraph with no
//     deactivated edge is one candidate whatever its connectivity (:342-343). A
//     candidate's id is its first node (min index), so ids sort in the reference's
//     candidate order (subgraph order, then weakly_connected_components order).
//  2. Members grouped per candidate by one radix sort of (candidate, order key).
//  3. One thread per candidate (a candidate is a handful of hits): fragment check,
//     close-proximity merging with the reference's in-place GNN_Measurement mutation
//     (:56-152), the one-hit-per-layer check (:407), the stable sort by radius (:411),
//     rotate_track (:176-195), the xy (3-state OU) and rz (2-state) Kalman fits with
//     filterpy 1.4.5 predict/update (:209-327) and the chi-square p-values
//     (scipy.stats.chi2.sf = the regularized upper incomplete gamma, cephes igamc).
//
// Around it, for a loop that stays in HBM (gtf.pipeline.run(resident="device")):
//  * gtf_candidate_order_device: the member order of step 2 as the reference builds it
//    (:332-346; gtf_candidate_order in gtf_build.cpp is the host form) -- the same hook +
//    compress rounds over the edges with act != 0, one sort for the members, ranks for
//    components of at least half their subgraph, one thread's BFS into a CPython set
//    (gtf_pyset.h) for the smaller ones;
//  * gtf_extract_outputs: the keep mask and the extracted / remaining / fragment lists
//    (:423-430, :459-467; gtf/extract.py outputs) by exclusive sums over the results and over
//    the sorted member list that step 2 left in the workspace.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdint.h>

#include "../../include/gtf.h"
#include "gtf_host.h"
#include "gtf_pyset.h"

namespace {

using gtf::bad;
using gtf::fail;
using gtf::grid;

constexpr int BLOCK = gtf::BLOCK256;

// ------------------------------------------------------------------ CCA
__global__ void __launch_bounds__(BLOCK) k_ex_init(int n, int n_sub, int32_t* label, uint8_t* inactive,
                                                   int32_t* flag) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < n) label[t] = t;
    if (t < n_sub) inactive[t] = 0;
    if (t == 0) *flag = 0;
}

__global__ void __launch_bounds__(BLOCK) k_ex_inactive(gtf_graph g, gtf_edges e, const int32_t* sub,
                                                       uint8_t* inactive) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= g.n_slots || !g.is_edge[k]) return;
    if (e.act[k] == 0) inactive[sub[g.slot_dst[k]]] = 1;   // :335-336 (activated == 0)
}

__device__ __forceinline__ int find_root(const int32_t* label, int x) {
    int p = label[x];
    while (p != x) {
        x = p;
        p = label[x];
    }
    return x;
}

// hook the larger root under the smaller one for every active edge (ANY: act != 0, the
// candidate order's rule -- gtf_candidate_order walks those; else act == 1, the extraction's)
template <bool ANY>
__global__ void __launch_bounds__(BLOCK) k_ex_hook(gtf_graph g, gtf_edges e, int32_t* label, int32_t* flag) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= g.n_slots || !g.is_edge[k] || (ANY ? e.act[k] == 0 : e.act[k] != 1)) return;
    const int u = g.slot_src[k], v = g.slot_dst[k];
    const int ru = find_root(label, u), rv = find_root(label, v);
    if (ru == rv) return;
    const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    atomicMin(&label[hi], lo);
    *flag = 1;
}

__global__ void __launch_bounds__(BLOCK) k_ex_compress(int n, int32_t* label) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v < n) label[v] = find_root(label, v);
}

// subgraphs without a deactivated edge stay whole; then the sort keys
__global__ void __launch_bounds__(BLOCK) k_ex_keys(int n, const int32_t* sub, const int32_t* sub_ptr,
                                                   const uint8_t* inactive, const int32_t* order_key,
                                                   int32_t* label, uint64_t* keys, int32_t* vals) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n) return;
    const int s = sub[v];
    int l = label[v];
    if (!inactive[s]) l = sub_ptr[s];
    label[v] = l;
    keys[v] = ((uint64_t)(uint32_t)l << 32) | (uint32_t)(order_key ? order_key[v] : v);
    vals[v] = v;
}

__global__ void __launch_bounds__(BLOCK) k_ex_starts(int n, const uint64_t* keys, int32_t* is_start) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) is_start[i] = (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1 : 0;
}

__global__ void __launch_bounds__(BLOCK) k_ex_ptr(int n, const int32_t* is_start, const int32_t* cidx,
                                                  int32_t* cand_ptr, int32_t* n_cand) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n && is_start[i]) cand_ptr[cidx[i]] = i;
    if (i == n - 1) {
        const int nc = cidx[i] + is_start[i];
        *n_cand = nc;
        cand_ptr[nc] = n;
    }
}

// ------------------------------------------------------------------ chi2.sf
constexpr double MACHEP = 1.11022302462515654042e-16;
constexpr double MAXLOG = 7.09782712893383996843e2;
constexpr double BIG = 4.503599627370496e15;
constexpr double BIGINV = 2.22044604925031308085e-16;

__device__ double igamc(double a, double x);

__device__ double igam(double a, double x) {
    if (x <= 0.0 || a <= 0.0) return 0.0;
    if (x > 1.0 && x > a) return 1.0 - igamc(a, x);
    double ax = a * log(x) - x - lgamma(a);
    if (ax < -MAXLOG) return 0.0;
    ax = exp(ax);
    double r = a, c = 1.0, ans = 1.0;
    do {
        r += 1.0;
        c *= x / r;
        ans += c;
    } while (c / ans > MACHEP);
    return ans * ax / a;
}

__device__ double igamc(double a, double x) {
    if (x < 0.0 || a <= 0.0) return NAN;
    if (x < 1.0 || x < a) return 1.0 - igam(a, x);
    double ax = a * log(x) - x - lgamma(a);
    if (ax < -MAXLOG) return 0.0;
    ax = exp(ax);
    double y = 1.0 - a, z = x + y + 1.0, c = 0.0;
    double pkm2 = 1.0, qkm2 = x, pkm1 = x + 1.0, qkm1 = z * x;
    double ans = pkm1 / qkm1, t;
    do {
        c += 1.0;
        y += 1.0;
        z += 2.0;
        const double yc = y * c;
        const double pk = pkm1 * z - pkm2 * yc;
        const double qk = qkm1 * z - qkm2 * yc;
        if (qk != 0.0) {
            const double r = pk / qk;
            t = fabs((ans - r) / r);
            ans = r;
        } else {
            t = 1.0;
        }
        pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;
        if (fabs(pk) > BIG) { pkm2 *= BIGINV; pkm1 *= BIGINV; qkm2 *= BIGINV; qkm1 *= BIGINV; }
    } while (t > MACHEP);
    return ans * ax;
}

__device__ __forceinline__ double chi2_sf(double x, int dof) {
    if (x != x) return NAN;
    return igamc(0.5 * dof, 0.5 * x);
}

// ------------------------------------------------------------------ CPython set order
// Iteration order of set() over the <= 2 duplicated (volume_id, in_volume_layer_id)
// tuples (:96): CPython 3.10 tuple hash (xxHash lanes of the item hashes; an integral
// float hashes to its integer) and set insertion into the minimum 8-slot table.
__device__ __forceinline__ uint64_t py_tuple_hash2(double a, double b) {
    const uint64_t P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P5 = 2870177450012600261ull;
    uint64_t acc = P5;
    const double it[2] = {a, b};
    for (int i = 0; i < 2; i++) {
        const int64_t hv = (int64_t)it[i];          // integral, small, non-negative
        const uint64_t lane = (uint64_t)(hv == -1 ? -2 : hv);
        acc += lane * P2;
        acc = (acc << 31) | (acc >> 33);
        acc *= P1;
    }
    acc += 2ull ^ (P5 ^ 3527539ull);
    if (acc == ~0ull) return 1546275796ull;
    return acc;
}

__device__ __forceinline__ int py_set_slot(uint64_t h, int occupied) {
    uint64_t i = h & 7ull, perturb = h;
    while ((int)i == occupied) {
        perturb >>= 5;
        i = (i * 5 + 1 + perturb) & 7ull;
    }
    return (int)i;
}

// ------------------------------------------------------------------ per candidate
struct Hit {
    double x, y, z, r;
};

struct KfState3 {
    double x[3], P[3][3];
};

// filterpy predict (x = F x, P = F P F^T + Q) and update with H = [1 0 0], scalar R
__device__ void kf3_step(KfState3& s, const double F[3][3], const double Q[3][3], double R, double z) {
    double x[3], FP[3][3], P[3][3];
    for (int i = 0; i < 3; i++) {
        double v = F[i][0] * s.x[0];
        v = v + F[i][1] * s.x[1];
        v = v + F[i][2] * s.x[2];
        x[i] = v;
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = F[i][0] * s.P[0][j];
            v = v + F[i][1] * s.P[1][j];
            v = v + F[i][2] * s.P[2][j];
            FP[i][j] = v;
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = FP[i][0] * F[j][0];
            v = v + FP[i][1] * F[j][1];
            v = v + FP[i][2] * F[j][2];
            P[i][j] = v + Q[i][j];
        }
    const double y = z - x[0];
    const double S = P[0][0] + R;
    const double SI = 1.0 / S;
    const double K[3] = {P[0][0] * SI, P[1][0] * SI, P[2][0] * SI};
    for (int i = 0; i < 3; i++) s.x[i] = x[i] + K[i] * y;
    // Joseph form: (I - K H) P (I - K H)^T + K R K^T
    double IKH[3][3] = {{1.0 - K[0], 0.0, 0.0}, {0.0 - K[1], 1.0, 0.0}, {0.0 - K[2], 0.0, 1.0}};
    double A[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = IKH[i][0] * P[0][j];
            v = v + IKH[i][1] * P[1][j];
            v = v + IKH[i][2] * P[2][j];
            A[i][j] = v;
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = A[i][0] * IKH[j][0];
            v = v + A[i][1] * IKH[j][1];
            v = v + A[i][2] * IKH[j][2];
            s.P[i][j] = v + (K[i] * R) * K[j];
        }
}

struct KfState2 {
    double x[2], P[2][2];
};

// F = [[1, dz], [0, 1]], scalar Q added to every entry of P (filterpy keeps a scalar Q
// as is, so F P F^T + Q broadcasts), H = [1 0], scalar R
__device__ void kf2_step(KfState2& s, double dz, double Q, double R, double z) {
    const double x0 = s.x[0] + dz * s.x[1], x1 = s.x[1];
    double FP[2][2];
    FP[0][0] = s.P[0][0] + dz * s.P[1][0];
    FP[0][1] = s.P[0][1] + dz * s.P[1][1];
    FP[1][0] = 0.0 * s.P[0][0] + 1.0 * s.P[1][0];
    FP[1][1] = 0.0 * s.P[0][1] + 1.0 * s.P[1][1];
    double P[2][2];
    P[0][0] = (FP[0][0] * 1.0 + FP[0][1] * dz) + Q;
    P[0][1] = (FP[0][0] * 0.0 + FP[0][1] * 1.0) + Q;
    P[1][0] = (FP[1][0] * 1.0 + FP[1][1] * dz) + Q;
    P[1][1] = (FP[1][0] * 0.0 + FP[1][1] * 1.0) + Q;
    const double y = z - x0;
    const double S = P[0][0] + R;
    const double SI = 1.0 / S;
    const double K[2] = {P[0][0] * SI, P[1][0] * SI};
    s.x[0] = x0 + K[0] * y;
    s.x[1] = x1 + K[1] * y;
    const double IKH[2][2] = {{1.0 - K[0], 0.0}, {0.0 - K[1], 1.0}};
    double A[2][2];
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) A[i][j] = IKH[i][0] * P[0][j] + IKH[i][1] * P[1][j];
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) s.P[i][j] = (A[i][0] * IKH[j][0] + A[i][1] * IKH[j][1]) + (K[i] * R) * K[j];
}

enum { EX_FRAGMENT = 0, EX_BAD = 1, EX_REJECTED = 2, EX_EXTRACTED = 3 };

__global__ void __launch_bounds__(BLOCK) k_ex_candidate(gtf_extract_io io, gtf_extract_params p,
                                                        const int32_t* members, const int32_t* cand_ptr,
                                                        const int32_t* n_cand_dev) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= *n_cand_dev) return;
    const int lo = cand_ptr[c], n = cand_ptr[c + 1] - lo;
    const int32_t* m = members + lo;
    const int root = io.label[m[0]];
    io.status[root] = EX_FRAGMENT;
    io.pval_xy[root] = NAN;
    io.pval_zr[root] = NAN;
    if (n < p.fragment) return;                                                   // :398
    auto vv = [&](int i, int comp) { return io.vivl[2 * (int64_t)m[i] + comp]; };
    auto same = [&](int i, int j) { return vv(i, 0) == vv(j, 0) && vv(i, 1) == vv(j, 1); };

    // ---- check_close_proximity_nodes (:56-152)
    int n2count = 0, bad_other = 0;
    int dup_first[2] = {-1, -1};
    for (int i = 0; i < n; i++) {
        bool first = true;
        int cnt = 0;
        for (int j = 0; j < n; j++) {
            if (same(i, j)) {
                cnt++;
                if (j < i) first = false;
            }
        }
        if (!first) continue;
        if (cnt == 2) {
            if (n2count < 2) dup_first[n2count] = i;
            n2count++;
        } else if (cnt != 1) {
            bad_other = 1;
        }
    }
    int removed[2] = {-1, -1}, mnode[2] = {-1, -1};
    Hit mid[2];
    bool copied = false;
    if (n2count >= 1 && n2count <= 2 && !bad_other) {
        copied = true;
        // set() iteration order of the duplicated tuples
        int order[2] = {0, 1};
        if (n2count == 2) {
            const uint64_t hA = py_tuple_hash2(vv(dup_first[0], 0), vv(dup_first[0], 1));
            const uint64_t hB = py_tuple_hash2(vv(dup_first[1], 0), vv(dup_first[1], 1));
            const int sA = py_set_slot(hA, -1);
            const int sB = py_set_slot(hB, sA);
            if (sB < sA) { order[0] = 1; order[1] = 0; }
        }
        int nm = 0;
        for (int q = 0; q < n2count; q++) {
            const int i1 = dup_first[order[q]];
            int i2 = -1;
            for (int j = i1 + 1; j < n && i2 < 0; j++)
                if (same(i1, j)) i2 = j;
            const double* c1 = io.xyzr + 4 * (int64_t)m[i1];
            const double* c2 = io.xyzr + 4 * (int64_t)m[i2];
            const double dx = c1[0] - c2[0], dy = c1[1] - c2[1], dz = c1[2] - c2[2];
            const double dist = sqrt(((dx * dx) + (dy * dy)) + (dz * dz));
            if (dist <= p.merge_distance) {
                Hit h;
                h.x = (c1[0] + c2[0]) / 2;
                h.y = (c1[1] + c2[1]) / 2;
                h.z = (c1[2] + c2[2]) / 2;
                h.r = sqrt(h.x * h.x + h.y * h.y);
                double* gm = io.gnn + 4 * (int64_t)m[i1];            // shared GNN_Measurement (:111-114)
                gm[0] = h.x; gm[1] = h.y; gm[2] = h.z; gm[3] = h.r;
                mnode[nm] = i1;
                mid[nm] = h;
                removed[nm] = i2;
                nm++;
            } else {
                copied = false;                                                  // :143-145
                break;
            }
        }
    }
    if (!copied) { removed[0] = removed[1] = -1; mnode[0] = mnode[1] = -1; }
    auto alive = [&](int i) { return i != removed[0] && i != removed[1]; };
    auto hit = [&](int i) {
        if (i == mnode[0]) return mid[0];
        if (i == mnode[1]) return mid[1];
        const double* c = io.xyzr + 4 * (int64_t)m[i];
        return Hit{c[0], c[1], c[2], c[3]};
    };

    // ---- one hit per layer (:405-407)
    int na = 0;
    bool unique = true;
    for (int i = 0; i < n; i++) {
        if (!alive(i)) continue;
        na++;
        for (int j = 0; j < i && unique; j++)
            if (alive(j) && same(i, j)) unique = false;
    }
    if (!unique || na < p.fragment) { io.status[root] = EX_BAD; return; }

    // ---- coordinates by radius, largest first, stable (:409-411): walk the order
    // with (r, position) cursors instead of sorting
    auto before = [&](int i, int j) {      // does i come before j in the sorted order?
        const double ri = hit(i).r, rj = hit(j).r;
        return ri > rj || (ri == rj && i < j);
    };
    auto next_after = [&](int last) {      // the element right after `last` (-1 = first)
        int best = -1;
        for (int i = 0; i < n; i++) {
            if (!alive(i)) continue;
            if (last >= 0 && !before(last, i)) continue;
            if (best < 0 || before(i, best)) best = i;
        }
        return best;
    };
    // the innermost three (coords[-1], [-2], [-3]) for rotate_track
    int last3[3] = {-1, -1, -1};
    for (int i = 0; i < n; i++) {
        if (!alive(i)) continue;
        // keep the 3 latest in order: last3[0] = last element, [1] = second last ...
        if (last3[0] < 0 || before(last3[0], i)) { last3[2] = last3[1]; last3[1] = last3[0]; last3[0] = i; }
        else if (last3[1] < 0 || before(last3[1], i)) { last3[2] = last3[1]; last3[1] = i; }
        else if (last3[2] < 0 || before(last3[2], i)) { last3[2] = i; }
    }
    const Hit p1 = hit(last3[0]);
    Hit p2 = hit(last3[1]);
    {
        const double dx = p1.x - p2.x, dy = p1.y - p2.y, dz = p1.z - p2.z;
        if (sqrt(((dx * dx) + (dy * dy)) + (dz * dz)) < p.separation_3d) p2 = hit(last3[2]);   // :181-183
    }
    const double axy = atan2(p2.y - p1.y, p2.x - p1.x), azr = atan2(p2.z - p1.z, p2.r - p1.r);
    const double cxy = cos(axy), sxy = sin(axy), czr = cos(azr), szr = sin(azr);
    auto rot = [&](const Hit& h) {
        return Hit{h.x * cxy + h.y * sxy, -h.x * sxy + h.y * cxy, -h.z * szr + h.z * czr, h.r * czr + h.r * szr};
    };

    // ---- KF_track_fit_moliere (:209-327)
    int cur = next_after(-1);
    Hit h2 = rot(hit(cur));
    KfState3 f;
    f.x[0] = h2.y; f.x[1] = 0.0; f.x[2] = 0.0;
    const double s2xy = p.sigma0xy * p.sigma0xy, s2rz = p.sigma0rz * p.sigma0rz;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) f.P[i][j] = 0.0;
    f.P[0][0] = s2xy; f.P[1][1] = 1.0; f.P[2][2] = 1.0;
    KfState2 gk;
    gk.x[0] = h2.r; gk.x[1] = 0.0;
    gk.P[0][0] = s2rz; gk.P[0][1] = 0.0; gk.P[1][0] = 0.0; gk.P[1][1] = 1000.0;
    double c2xy = 0.0, c2zr = 0.0;
    for (int step = 0; step < na - 1; step++) {
        cur = next_after(cur);
        const Hit h3 = rot(hit(cur));
        const double x1 = 0.0, y1 = 0.0;
        const double x2 = h2.x, y2 = h2.y, x3 = h3.x, y3 = h3.y;
        const double denom = (x1 - x2) * (x1 - x3) * (x2 - x3);
        const double a = ((x3 * (y2 - y1)) + (x2 * (y1 - y3)) + (x1 * (y3 - y2))) / denom;
        const double b = ((x3 * x3 * (y1 - y2)) + (x2 * x2 * (y3 - y1)) + (x1 * x1 * (y2 - y3))) / denom;
        const double dr = h3.r - h2.r, dz = h3.z - h2.z;
        const double hyp = sqrt(dr * dr + dz * dz);
        const double sin_t = fabs(dr) / hyp;
        const double q = (2.0 * a * x3) + b;
        const double t15 = 1.0 + q * q;
        const double kappa = (2.0 * a) / (t15 * sqrt(t15));
        const double hl = (13.6 * 1e-3 * sqrt(0.02) * kappa) / 0.3;
        double var_ms = sin_t * (hl * hl);
        if (fabs(h3.z) >= p.endcap_boundary) var_ms = var_ms * fabs(dr / dz);
        const double dx = x3 - x2;
        const double alpha = 0.1;
        const double e1 = exp(-fabs(dx) * alpha);
        const double f1 = (1.0 - e1) / alpha;
        const double g1 = (fabs(dx) - f1) / alpha;
        const double sw2 = 0.00001 * 0.00001, st2 = var_ms;
        const double dx2 = dx * dx, dxw2 = dx2 * sw2;
        const double Q02 = 0.5 * dxw2, Q01 = dx * (st2 + Q02), Q12 = dx * sw2;
        const double F[3][3] = {{1.0, dx, g1}, {0.0, 1.0, f1}, {0.0, 0.0, e1}};
        const double Q[3][3] = {{dx2 * (st2 + 0.25 * dxw2), Q01, Q02}, {Q01, st2 + dxw2, Q12}, {Q02, Q12, sw2}};
        kf3_step(f, F, Q, s2xy, y3);
        {
            const double res = y3 - f.x[0];
            const double S = f.P[0][0] + s2xy;
            c2xy = c2xy + (res * (1.0 / S)) * res;
        }
        kf2_step(gk, dz, var_ms, s2rz, h3.r);
        {
            const double res = h3.r - gk.x[0];
            const double S = gk.P[0][0] + s2rz;
            c2zr = c2zr + (res * (1.0 / S)) * res;
        }
        h2 = h3;
    }
    const double pv = chi2_sf(c2xy, na - 2), pz = chi2_sf(c2zr, na - 2);
    io.pval_xy[root] = pv;
    io.pval_zr[root] = pz;
    io.status[root] = (pv >= p.p_accept && pz >= p.p_accept) ? EX_EXTRACTED : EX_REJECTED;     // :416
}

__global__ void __launch_bounds__(BLOCK) k_ex_flags(int n, gtf_extract_io io) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v < n) io.extracted[v] = io.status[io.label[v]] == EX_EXTRACTED ? 1 : 0;
}

// label[v] = v, the subgraphs' inactive flags, then hook + compress until no root changes
// (candidates are short: a few rounds; one stream synchronisation per round): every
// component ends labelled by its minimum node index. 0, or -1 with the error set.
template <bool ANY>
int cca_rounds(const gtf_graph* g, const gtf_edges* e, const int32_t* sub_id, int n_sub, int32_t* label,
               uint8_t* inactive, int32_t* flag, hipStream_t st, const char* who) {
    const int n = g->n_nodes;
    const int nb = grid(n > n_sub ? n : n_sub);
    hipLaunchKernelGGL(k_ex_init, dim3(nb), dim3(BLOCK), 0, st, n, n_sub, label, inactive, flag);
    if (g->n_slots > 0)
        hipLaunchKernelGGL(k_ex_inactive, dim3(grid(g->n_slots)), dim3(BLOCK), 0, st, *g, *e, sub_id, inactive);
    int32_t changed = 0;
    hipError_t err;
    for (int round = 0; round < 64; round++) {
        int32_t zero = 0;
        if ((err = hipMemcpyAsync(flag, &zero, sizeof(int32_t), hipMemcpyHostToDevice, st)) != hipSuccess)
            return fail(who, "CCA round", err);
        if (g->n_slots > 0)
            hipLaunchKernelGGL(k_ex_hook<ANY>, dim3(grid(g->n_slots)), dim3(BLOCK), 0, st, *g, *e, label, flag);
        hipLaunchKernelGGL(k_ex_compress, dim3(grid(n)), dim3(BLOCK), 0, st, n, label);
        if ((err = hipMemcpyAsync(&changed, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (err = hipStreamSynchronize(st)) != hipSuccess)
            return fail(who, "CCA round", err);
        if (!changed) break;
    }
    if (changed) {
        char m[120];
        snprintf(m, sizeof(m), "%s: CCA did not converge", who);
        gtf::set_error(m);
        return -1;
    }
    return 0;
}

// the hipcub calls of the extraction: one sort of (key, member) pairs, one scan of the starts
gtf::CubNeed ex_cub_need(int n) { return gtf::CubNeed().sort_pairs<uint64_t, int32_t>(n).scan<int32_t>(n); }

struct ExWs {
    uint64_t *keys_in, *keys_out;
    int32_t *vals_in, *vals_out, *is_start, *cidx, *cand_ptr, *flag;
    uint8_t* inactive;
    gtf::Scratch cub;
    size_t total;
};

// n >= 1
ExWs carve_ex(const void* base, int n, int n_sub) {
    gtf::Arena a(base);
    ExWs w;
    w.keys_in = a.take<uint64_t>(n);
    w.keys_out = a.take<uint64_t>(n);
    w.vals_in = a.take<int32_t>(n);
    w.vals_out = a.take<int32_t>(n);
    w.is_start = a.take<int32_t>(n);
    w.cidx = a.take<int32_t>(n);
    w.cand_ptr = a.take<int32_t>((size_t)n + 1);
    w.flag = a.take<int32_t>(1);
    w.inactive = a.take<uint8_t>(n_sub > 0 ? n_sub : 1);
    w.cub = ex_cub_need(n).take(a);
    w.total = a.used() + 256;
    return w;
}

// ------------------------------------------------------------------ sub_ptr
// sub_id must read 0, 1, 2, ... grouped: each first node of a subgraph writes its pointer;
// err is sub_ptr[n_sub], preset to N and overwritten only by a violation
__global__ void __launch_bounds__(BLOCK) k_sub_ptr(int n, int n_sub, const int32_t* sub, int32_t* sub_ptr,
                                                   int32_t* err) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n) return;
    const int s = sub[v], before = v ? sub[v - 1] : -1;
    if (s < 0 || s >= n_sub || (s != before && s != before + 1) || (v == n - 1 && s != n_sub - 1)) {
        *err = -1;         // (every writer stores the same value)
        return;
    }
    if (s != before) sub_ptr[s] = v;
}

// ------------------------------------------------------------------ candidate order
constexpr int32_t OERR_RANGE = 1, OERR_DUP = 2, OERR_OVER = 4;
enum { OS_ERR = 0, OS_NCOMP = 1, OS_NSET = 2, OS_MAXSET = 3, OS_WORDS = 4 };

__global__ void __launch_bounds__(BLOCK) k_ord_keys(int n, const int32_t* label, uint64_t* keys, int32_t* vals,
                                                    uint8_t* seen) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n) return;
    keys[v] = ((uint64_t)(uint32_t)label[v] << 32) | (uint32_t)v;
    vals[v] = v;
    seen[v] = 0;
}

// the sorted ids: range (a negative id is a huge unsigned one) and duplicates
// (evs: the events beside the ids sorted by (event, id), or NULL: equal ids of two events are no duplicate)
__global__ void __launch_bounds__(BLOCK) k_ord_check_ids(int n, const uint64_t* ids, const uint32_t* evs, int32_t* err) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (ids[i] >= ((uint64_t)1 << 61) - 1) atomicOr(err, OERR_RANGE);      // (only on a violation)
    if (i > 0 && ids[i] == ids[i - 1] && (!evs || evs[i] == evs[i - 1])) atomicOr(err, OERR_DUP);
}

// a batch of events: the event of every entry of the id-sorted map, the key of the second (stable) sort
__global__ void __launch_bounds__(BLOCK) k_ord_ev_keys(int n, const int32_t* event, const int32_t* idx, uint32_t* keys) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = idx[i];
    keys[i] = v >= 0 && v < n ? (uint32_t)event[v] : 0u;
}

// ... and the ids in the final (event, id) order
__global__ void __launch_bounds__(BLOCK) k_ord_ev_ids(int n, const int64_t* node_id, const int32_t* idx, uint64_t* ids) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = idx[i];
    ids[i] = v >= 0 && v < n ? (uint64_t)node_id[v] : ~(uint64_t)0;
}

// find_id (gtf_pyset.h) in a map sorted by (event, id): the node of event `ev` with this id, or -1
__device__ inline int32_t find_id_ev(const uint32_t* evs, const uint64_t* ids, const int32_t* idx, int32_t n, uint32_t ev,
                                     int64_t key) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t m = (lo + hi) >> 1;
        if (evs[m] < ev || (evs[m] == ev && ids[m] < (uint64_t)key)) lo = m + 1;
        else hi = m;
    }
    return (lo < n && evs[lo] == ev && ids[lo] == (uint64_t)key) ? idx[lo] : -1;
}

// is component c (< n_comp) ordered by the set walk? its subgraph has an inactive edge and
// it holds fewer than half the subgraph's nodes
__device__ __forceinline__ bool set_ordered(int c, const int32_t* cptr, const int32_t* memb, const int32_t* sub,
                                            const int32_t* sub_ptr, const uint8_t* inactive) {
    const int s = sub[memb[cptr[c]]];
    return inactive[s] && 2 * (int64_t)(cptr[c + 1] - cptr[c]) < (int64_t)(sub_ptr[s + 1] - sub_ptr[s]);
}

// per component slot c in [0, n]: the words of its three set tables (0 when it is not
// set-ordered or c >= n_comp), the flag and the size for the counts
__global__ void __launch_bounds__(BLOCK) k_ord_words(int n, const int32_t* n_comp, const int32_t* cptr,
                                                     const int32_t* memb, const int32_t* sub,
                                                     const int32_t* sub_ptr, const uint8_t* inactive,
                                                     int64_t* words, int32_t* so_flag, int32_t* so_size) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c > n) return;
    const bool so = c < *n_comp && set_ordered(c, cptr, memb, sub, sub_ptr, inactive);
    const int sz = so ? cptr[c + 1] - cptr[c] : 0;
    words[c] = so ? 3 * set_capacity(sz) : 0;
    if (c < n) {
        so_flag[c] = so ? 1 : 0;
        so_size[c] = sz;
    }
}

// every node by its position i in the sorted member list: the whole subgraph's node order,
// or the rank among the component's members; set-ordered components are left to k_ord_walk
__global__ void __launch_bounds__(BLOCK) k_ord_rank(int n, const int32_t* memb, const int32_t* is_start,
                                                    const int32_t* cidx, const int32_t* cptr, const int32_t* sub,
                                                    const int32_t* sub_ptr, const uint8_t* inactive,
                                                    int32_t* order_key) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = memb[i], s = sub[v];
    if (!inactive[s]) { order_key[v] = v - sub_ptr[s]; return; }                     // :342-343
    const int c = cidx[i] + is_start[i] - 1;
    if (2 * (int64_t)(cptr[c + 1] - cptr[c]) >= (int64_t)(sub_ptr[s + 1] - sub_ptr[s])) order_key[v] = i - cptr[c];
}

// one thread per set-ordered component: nx.weakly_connected_components' set(_plain_bfs(G, root))
// from the component's first node -- per level node the successors in out_slot order, then the
// predecessors in slot order, over edges with act != 0 -- then the copy's node order = the
// order of a second set filled from the first (show_nodes(set(c))). The queue is the
// component's own segment of an N-long array.
__global__ void __launch_bounds__(BLOCK) k_ord_walk(gtf_graph g, const uint8_t* act, int n, const int32_t* n_comp,
                                                    const int32_t* cptr, const int32_t* memb,
                                                    const int32_t* so_flag, const int64_t* node_id,
                                                    const int32_t* event, const uint32_t* evs,
                                                    const uint64_t* ids, const int32_t* idx, const int64_t* toff,
                                                    int64_t* tbl, int64_t tbl_words, int32_t* queue, uint8_t* seen,
                                                    int32_t* order_key, int32_t* err) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= *n_comp || !so_flag[c]) return;
    const int32_t lo = cptr[c], sz = cptr[c + 1] - lo;
    const int64_t cap = set_capacity(sz);
    if (toff[c] + 3 * cap > tbl_words) { atomicOr(err, OERR_OVER); return; }
    int64_t* t = tbl + toff[c];
    DevSet s;
    s.init(t, t + cap, cap);
    const int32_t root = memb[lo];
    int32_t head = lo, tail = lo;
    bool full = false;
    auto visit = [&](int32_t w) {
        if (seen[w]) return;
        if (tail >= lo + sz) { full = true; return; }     // (cannot happen: the walk and the hooks use one edge rule)
        seen[w] = 1;
        s.add(node_id[w]);
        queue[tail++] = w;
    };
    visit(root);
    while (head < tail && !full) {
        const int32_t v = queue[head++];
        for (int32_t j = g.out_ptr[v]; j < g.out_ptr[v + 1]; j++) {
            const int32_t k = g.out_slot[j];
            if (act[k] != 0) visit(g.slot_dst[k]);                         // successors, G order
        }
        for (int32_t k = g.slot_ptr[v]; k < g.slot_ptr[v + 1]; k++)
            if (g.is_edge[k] && act[k] != 0) visit(g.slot_src[k]);        // predecessors
    }
    DevSet shown;
    int64_t* spare = (s.a == t) ? t + cap : t;   // the first set's spare table
    shown.init(spare, t + 2 * cap, cap);
    for (int64_t i = 0; i <= s.mask; i++)
        if (s.a[i] >= 0) shown.add(s.a[i]);
    if (full || s.over || shown.over) { atomicOr(err, OERR_OVER); return; }
    int32_t r = 0;
    for (int64_t i = 0; i <= shown.mask; i++) {
        if (shown.a[i] < 0) continue;
        const int32_t v = event ? find_id_ev(evs, ids, idx, n, (uint32_t)event[root], shown.a[i])
                                : find_id(ids, idx, n, shown.a[i]);
        if (v >= 0) order_key[v] = r;
        r++;
    }
}

struct OrdWs {
    uint64_t *keys_in, *keys_out, *ids;
    int32_t *vals_in, *memb, *idx, *is_start, *cidx, *cptr, *label, *queue, *so_flag, *so_size, *scal;
    int64_t *words, *toff, *tbl;
    uint8_t *seen, *inactive;
    gtf::Scratch cub;
    size_t tbl_words, total;
};

// n >= 1. The set tables: a set of k distinct keys has a table of <= 8 max(k, 1) entries and a
// component takes three, so <= 24 N words (the bound argued in gtf_build_dev.hip's carve)
OrdWs carve_ord(void* base, int n, int n_sub) {
    gtf::Arena a(base);
    OrdWs w;
    const size_t n1 = (size_t)n + 1;
    w.keys_in = a.take<uint64_t>(n);
    w.keys_out = a.take<uint64_t>(n);
    w.ids = a.take<uint64_t>(n);
    w.words = a.take<int64_t>(n1);
    w.toff = a.take<int64_t>(n1);
    w.vals_in = a.take<int32_t>(n);
    w.memb = a.take<int32_t>(n);
    w.idx = a.take<int32_t>(n);
    w.is_start = a.take<int32_t>(n);
    w.cidx = a.take<int32_t>(n);
    w.cptr = a.take<int32_t>(n1);
    w.label = a.take<int32_t>(n);
    w.queue = a.take<int32_t>(n);
    w.so_flag = a.take<int32_t>(n);
    w.so_size = a.take<int32_t>(n);
    w.scal = a.take<int32_t>(16);
    w.seen = a.take<uint8_t>(n);
    w.inactive = a.take<uint8_t>(n_sub > 0 ? n_sub : 1);
    w.cub = ex_cub_need(n).sort_pairs<uint32_t, int32_t>(n).scan<int64_t>(n + 1).sum<int32_t>(n).max<int32_t>(n).take(a);
    w.tbl_words = 24 * (size_t)n;
    w.tbl = a.take<int64_t>(w.tbl_words);
    w.total = a.used() + 256;
    return w;
}

// ------------------------------------------------------------------ outputs
__global__ void __launch_bounds__(BLOCK) k_out_notext(int n, const uint8_t* extracted, int32_t* notext) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v <= n) notext[v] = (v < n && !extracted[v]) ? 1 : 0;
}

// per subgraph: left, and (1 << 32 | left) where it is a remaining / a fragment subgraph, so
// one 64-bit exclusive sum gives both the subgraph's place in its list and its first node's
__global__ void __launch_bounds__(BLOCK) k_out_sub(int n_sub, int fragment, const int32_t* sub_ptr,
                                                   const int32_t* pre, int32_t* left, int64_t* rem, int64_t* frag) {
    const int s = blockIdx.x * BLOCK + threadIdx.x;
    if (s > n_sub) return;
    const int l = s < n_sub ? pre[sub_ptr[s + 1]] - pre[sub_ptr[s]] : 0;
    if (s < n_sub) left[s] = l;
    rem[s] = l >= fragment ? ((int64_t)1 << 32) | l : 0;
    frag[s] = (l > 0 && l < fragment) ? ((int64_t)1 << 32) | l : 0;
}

__global__ void __launch_bounds__(BLOCK) k_out_cand(int n, const int32_t* n_cand, const int32_t* cand_ptr,
                                                    const int32_t* members, const int32_t* label,
                                                    const int8_t* status, int64_t* ext) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c > n) return;
    int64_t e = 0;
    if (c < *n_cand && status[label[members[cand_ptr[c]]]] == EX_EXTRACTED)
        e = ((int64_t)1 << 32) | (cand_ptr[c + 1] - cand_ptr[c]);
    ext[c] = e;
}

__global__ void __launch_bounds__(BLOCK) k_out_nodes(int n, int n_sub, int fragment, gtf_extract_io io,
                                                     gtf_extract_out o, const int32_t* pre, const int64_t* rem,
                                                     const int64_t* frag) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n) return;
    const int s = io.sub_id[v];
    const int l = o.left[s];
    const bool kept = !io.extracted[v] && l >= fragment;
    o.keep[v] = kept ? 1 : 0;
    if (io.extracted[v] || l == 0) return;
    const int at = pre[v] - pre[io.sub_ptr[s]];          // among the subgraph's nodes that stay
    const bool first = at == 0;
    if (l >= fragment) {
        const int pos = (int)(rem[s] & 0xffffffff) + at;
        if (o.rem_nodes) o.rem_nodes[pos] = v;
        if (o.rem_ids) o.rem_ids[pos] = o.node_id[v];
        if (first && o.rem_ptr) o.rem_ptr[rem[s] >> 32] = pos;
    } else {
        const int pos = (int)(frag[s] & 0xffffffff) + at;
        if (o.frag_nodes) o.frag_nodes[pos] = v;
        if (o.frag_ids) o.frag_ids[pos] = o.node_id[v];
        if (first && o.frag_ptr) o.frag_ptr[frag[s] >> 32] = pos;
    }
}

// every position i of the extraction's sorted member list
__global__ void __launch_bounds__(BLOCK) k_out_members(int n, gtf_extract_io io, gtf_extract_out o,
                                                       const int32_t* members, const int32_t* is_start,
                                                       const int32_t* cidx, const int32_t* cand_ptr,
                                                       const int64_t* ext) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int c = cidx[i] + is_start[i] - 1;
    if (ext[c + 1] == ext[c]) return;                    // not extracted
    const int v = members[i];
    const int pos = (int)(ext[c] & 0xffffffff) + (i - cand_ptr[c]);
    if (o.cand_members) o.cand_members[pos] = v;
    if (o.cand_ids) o.cand_ids[pos] = o.node_id[v];
    if (is_start[i]) {
        const int k = (int)(ext[c] >> 32), root = io.label[v];
        if (o.cand_ptr) o.cand_ptr[k] = pos;
        if (o.pval_xy) o.pval_xy[k] = io.pval_xy[root];
        if (o.pval_zr) o.pval_zr[k] = io.pval_zr[root];
    }
}

// the six counts, and the closing pointer of every list
__global__ void k_out_counts(int n, int n_sub, gtf_extract_out o, const int64_t* ext, const int64_t* rem,
                             const int64_t* frag, int32_t* counts) {
    if (blockIdx.x || threadIdx.x) return;
    const int64_t t[3] = {ext[n], rem[n_sub], frag[n_sub]};
    int32_t* ptr[3] = {o.cand_ptr, o.rem_ptr, o.frag_ptr};
    for (int k = 0; k < 3; k++) {
        counts[2 * k] = (int32_t)(t[k] >> 32);
        counts[2 * k + 1] = (int32_t)(t[k] & 0xffffffff);
        if (ptr[k]) ptr[k][t[k] >> 32] = (int32_t)(t[k] & 0xffffffff);
    }
}

struct OutWs {
    int32_t *notext, *pre, *scal;
    int64_t *in64, *ext, *rem, *frag, *frag_in;
    gtf::Scratch cub;
    size_t total;
};

OutWs carve_out(void* base, int n, int n_sub) {
    gtf::Arena a(base);
    OutWs w;
    const size_t n1 = (size_t)n + 1, s1 = (size_t)n_sub + 1, m1 = n1 > s1 ? n1 : s1;
    w.in64 = a.take<int64_t>(m1);
    w.frag_in = a.take<int64_t>(s1);
    w.ext = a.take<int64_t>(n1);
    w.rem = a.take<int64_t>(s1);
    w.frag = a.take<int64_t>(s1);
    w.notext = a.take<int32_t>(n1);
    w.pre = a.take<int32_t>(n1);
    w.scal = a.take<int32_t>(16);
    w.cub = gtf::CubNeed().scan<int32_t>((int)m1).scan<int64_t>((int)m1).take(a);
    w.total = a.used() + 256;
    return w;
}

}  // namespace

extern "C" {

int gtf_subgraph_ptr_device(const int32_t* sub_id, int32_t n_nodes, int32_t n_sub, int32_t* sub_ptr,
                            gtf_stream_t stream) {
    const char* who = "gtf_subgraph_ptr_device";
    if (!sub_ptr || n_nodes < 0 || n_sub < 0 || (n_nodes && !sub_id) || (n_nodes > 0 && n_sub == 0))
        return bad("gtf_subgraph_ptr_device: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    hipError_t err;
    if (n_nodes == 0) {
        if ((err = hipMemsetAsync(sub_ptr, 0, 4 * ((size_t)n_sub + 1), st)) != hipSuccess) return fail(who, "memset", err);
        return 0;
    }
    int32_t last = n_nodes;
    const hipError_t set = hipMemcpyAsync(sub_ptr + n_sub, &last, 4, hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(k_sub_ptr, dim3(grid(n_nodes)), dim3(BLOCK), 0, st, n_nodes, n_sub, sub_id, sub_ptr,
                       sub_ptr + n_sub);
    if ((err = set) != hipSuccess ||
        (err = hipMemcpyAsync(&last, sub_ptr + n_sub, 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (err = hipStreamSynchronize(st)) != hipSuccess)
        return fail(who, "launch", err);
    if (last != n_nodes)
        return bad("gtf_subgraph_ptr_device: sub_id must number the subgraphs 0 .. n_sub - 1 with the nodes grouped");
    return 0;
}

size_t gtf_candidate_order_workspace_bytes(int32_t n_nodes, int32_t n_slots, int32_t n_sub) {
    (void)n_slots;    // (the slot arrays are read in place)
    return carve_ord(nullptr, n_nodes > 0 ? n_nodes : 1, n_sub > 0 ? n_sub : 0).total;
}

int gtf_candidate_order_device(const gtf_graph* g, const gtf_edges* e, const int32_t* sub_id,
                               const int32_t* sub_ptr, int32_t n_sub, const int64_t* node_id,
                               int32_t* order_key, void* workspace, size_t workspace_bytes,
                               gtf_order_counts* counts, gtf_stream_t stream) {
    return gtf_candidate_order_device_ev(g, e, sub_id, sub_ptr, n_sub, node_id, nullptr, order_key, workspace,
                                         workspace_bytes, counts, stream);
}

// (the messages name gtf_candidate_order_device with or without events: one rule, one text)
int gtf_candidate_order_device_ev(const gtf_graph* g, const gtf_edges* e, const int32_t* sub_id,
                                  const int32_t* sub_ptr, int32_t n_sub, const int64_t* node_id,
                                  const int32_t* event, int32_t* order_key, void* workspace,
                                  size_t workspace_bytes, gtf_order_counts* counts, gtf_stream_t stream) {
    const char* who = "gtf_candidate_order_device";
    if (int rc = gtf::check_abi(g, who)) return rc;
    if (!e || !counts || !workspace || g->n_nodes < 0 || g->n_slots < 0 || g->n_edges < 0 || n_sub < 0)
        return bad("gtf_candidate_order_device: null argument or negative size");
    *counts = gtf_order_counts{0, 0, 0, 0};
    const int n = g->n_nodes;
    if (n == 0) return 0;
    if (!sub_id || !sub_ptr || !node_id || !order_key || !g->slot_ptr || !g->out_ptr ||
        (g->n_slots && (!g->slot_src || !g->slot_dst || !g->is_edge || !e->act)) || (g->n_edges && !g->out_slot))
        return bad("gtf_candidate_order_device: missing array (slot_ptr, slot_src, slot_dst, out_ptr, out_slot, "
                   "is_edge, act, sub_id, sub_ptr, node_id, order_key)");
    if (workspace_bytes < gtf_candidate_order_workspace_bytes(n, g->n_slots, n_sub))
        return bad("gtf_candidate_order_device: workspace smaller than gtf_candidate_order_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    const OrdWs w = carve_ord(workspace, n, n_sub);
    const gtf::Cub cub{w.cub, st};
    hipError_t err;
    if ((err = hipMemsetAsync(w.scal, 0, 64, st)) != hipSuccess) return fail(who, "memset", err);
    if (int rc = cca_rounds<true>(g, e, sub_id, n_sub, w.label, w.inactive, w.scal + 8, st, who)) return rc;
    // members of every component in node order, the component pointers and their count
    hipLaunchKernelGGL(k_ord_keys, dim3(grid(n)), dim3(BLOCK), 0, st, n, w.label, w.keys_in, w.vals_in, w.seen);
    if ((err = cub.sort_pairs(w.keys_in, w.keys_out, w.vals_in, w.memb, n)) != hipSuccess)
        return fail(who, "sort members", err);
    hipLaunchKernelGGL(k_ex_starts, dim3(grid(n)), dim3(BLOCK), 0, st, n, w.keys_out, w.is_start);
    if ((err = cub.scan(w.is_start, w.cidx, n)) != hipSuccess) return fail(who, "scan", err);
    hipLaunchKernelGGL(k_ex_ptr, dim3(grid(n)), dim3(BLOCK), 0, st, n, w.is_start, w.cidx, w.cptr, w.scal + OS_NCOMP);
    hipLaunchKernelGGL(k_ord_rank, dim3(grid(n)), dim3(BLOCK), 0, st, n, w.memb, w.is_start, w.cidx, w.cptr, sub_id,
                       sub_ptr, w.inactive, order_key);
    // node id -> index (keys_in is free again; vals_in still holds 0 .. n - 1)
    uint32_t* evs = nullptr;
    if (!event) {
        if ((err = cub.sort_pairs((const uint64_t*)node_id, w.ids, w.vals_in, w.idx, n)) != hipSuccess)
            return fail(who, "sort ids", err);
    } else {
        // by id, then stably by event: the map in (event, id) order. keys_out (its starts are taken) holds the
        // two arrays of event keys, the walk's queue the map between the sorts.
        uint32_t* ev_in = (uint32_t*)w.keys_out;
        evs = ev_in + n;
        if ((err = cub.sort_pairs((const uint64_t*)node_id, w.keys_in, w.vals_in, w.queue, n)) != hipSuccess)
            return fail(who, "sort ids", err);
        hipLaunchKernelGGL(k_ord_ev_keys, dim3(grid(n)), dim3(BLOCK), 0, st, n, event, w.queue, ev_in);
        if ((err = cub.sort_pairs(ev_in, evs, w.queue, w.idx, n)) != hipSuccess) return fail(who, "sort events", err);
        hipLaunchKernelGGL(k_ord_ev_ids, dim3(grid(n)), dim3(BLOCK), 0, st, n, node_id, w.idx, w.ids);
    }
    hipLaunchKernelGGL(k_ord_check_ids, dim3(grid(n)), dim3(BLOCK), 0, st, n, w.ids, evs, w.scal + OS_ERR);
    // the set-ordered components: table offsets and counts by scans, then one thread each
    hipLaunchKernelGGL(k_ord_words, dim3(grid(n + 1)), dim3(BLOCK), 0, st, n, w.scal + OS_NCOMP, w.cptr, w.memb,
                       sub_id, sub_ptr, w.inactive, w.words, w.so_flag, w.so_size);
    if ((err = cub.scan(w.words, w.toff, n + 1)) != hipSuccess) return fail(who, "scan", err);
    if ((err = cub.sum(w.so_flag, w.scal + OS_NSET, n)) != hipSuccess) return fail(who, "sum", err);
    if ((err = cub.max(w.so_size, w.scal + OS_MAXSET, n)) != hipSuccess) return fail(who, "max", err);
    hipLaunchKernelGGL(k_ord_walk, dim3(grid(n)), dim3(BLOCK), 0, st, *g, e->act, n, w.scal + OS_NCOMP, w.cptr, w.memb,
                       w.so_flag, node_id, event, evs, w.ids, w.idx, w.toff, w.tbl, (int64_t)w.tbl_words, w.queue, w.seen,
                       order_key, w.scal + OS_ERR);
    if ((err = hipGetLastError()) != hipSuccess) return fail(who, "launch", err);
    int32_t scal[4];
    if ((err = hipMemcpyAsync(scal, w.scal, sizeof(scal), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(who, "read", err);
    if ((err = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", err);
    if (scal[OS_ERR] & OERR_RANGE) return bad("gtf_candidate_order_device: node ids must be in [0, 2^61 - 1)");
    if (scal[OS_ERR] & OERR_DUP) return bad("gtf_candidate_order_device: duplicate node id");
    if (scal[OS_ERR] & OERR_OVER) {
        gtf::set_error("gtf_candidate_order_device: a set held more keys than its table was sized for");
        return -1;
    }
    *counts = gtf_order_counts{scal[OS_NCOMP], scal[OS_NSET], scal[OS_MAXSET], 0};
    return 0;
}

size_t gtf_extract_outputs_workspace_bytes(int32_t n_nodes, int32_t n_sub) {
    return carve_out(nullptr, n_nodes > 0 ? n_nodes : 1, n_sub > 0 ? n_sub : 0).total;
}

int gtf_extract_outputs(const gtf_graph* g, const gtf_extract_io* io, int32_t fragment,
                        const void* extract_workspace, const gtf_extract_out* out, void* workspace,
                        size_t workspace_bytes, gtf_extract_out_counts* counts, gtf_stream_t stream) {
    const char* who = "gtf_extract_outputs";
    if (int rc = gtf::check_abi(g, who)) return rc;
    if (!io || !out || !counts || !workspace || !extract_workspace || g->n_nodes < 0 || fragment < 1)
        return bad("gtf_extract_outputs: null argument, negative size or fragment < 1");
    *counts = gtf_extract_out_counts{0, 0, 0, 0, 0, 0};
    const int n = g->n_nodes, n_sub = io->n_sub;
    if (n == 0) return 0;
    if (!io->sub_id || !io->sub_ptr || !io->label || !io->status || !io->pval_xy || !io->pval_zr || !io->extracted ||
        !io->n_candidates || n_sub <= 0 || !out->left || !out->keep ||
        ((out->cand_ids || out->rem_ids || out->frag_ids) && !out->node_id))
        return bad("gtf_extract_outputs: missing arrays (the results of gtf_extract_candidates, left, keep, "
                   "node_id for the id lists)");
    if (workspace_bytes < gtf_extract_outputs_workspace_bytes(n, n_sub))
        return bad("gtf_extract_outputs: workspace smaller than gtf_extract_outputs_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    const ExWs x = carve_ex(extract_workspace, n, n_sub);
    const OutWs w = carve_out(workspace, n, n_sub);
    const gtf::Cub cub{w.cub, st};
    hipError_t err;
    // nodes that stay, counted before every node: left[s] is a difference at sub_ptr
    hipLaunchKernelGGL(k_out_notext, dim3(grid(n + 1)), dim3(BLOCK), 0, st, n, io->extracted, w.notext);
    if ((err = cub.scan(w.notext, w.pre, n + 1)) != hipSuccess) return fail(who, "scan", err);
    hipLaunchKernelGGL(k_out_sub, dim3(grid(n_sub + 1)), dim3(BLOCK), 0, st, n_sub, fragment, io->sub_ptr, w.pre,
                       out->left, w.in64, w.frag_in);
    if ((err = cub.scan(w.in64, w.rem, n_sub + 1)) != hipSuccess) return fail(who, "scan", err);
    if ((err = cub.scan(w.frag_in, w.frag, n_sub + 1)) != hipSuccess) return fail(who, "scan", err);
    hipLaunchKernelGGL(k_out_nodes, dim3(grid(n)), dim3(BLOCK), 0, st, n, n_sub, fragment, *io, *out, w.pre, w.rem,
                       w.frag);
    // the extracted candidates, in the order the extraction's sort left them
    hipLaunchKernelGGL(k_out_cand, dim3(grid(n + 1)), dim3(BLOCK), 0, st, n, io->n_candidates, x.cand_ptr, x.vals_out,
                       io->label, io->status, w.in64);
    if ((err = cub.scan(w.in64, w.ext, n + 1)) != hipSuccess) return fail(who, "scan", err);
    hipLaunchKernelGGL(k_out_members, dim3(grid(n)), dim3(BLOCK), 0, st, n, *io, *out, x.vals_out, x.is_start, x.cidx,
                       x.cand_ptr, w.ext);
    hipLaunchKernelGGL(k_out_counts, dim3(1), dim3(64), 0, st, n, n_sub, *out, w.ext, w.rem, w.frag, w.scal);
    if ((err = hipGetLastError()) != hipSuccess) return fail(who, "launch", err);
    int32_t c[6];
    if ((err = hipMemcpyAsync(c, w.scal, sizeof(c), hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "read", err);
    if ((err = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", err);
    *counts = gtf_extract_out_counts{c[0], c[1], c[2], c[3], c[4], c[5]};
    return 0;
}

size_t gtf_extract_workspace_bytes(int32_t n_nodes, int32_t n_sub) {
    return carve_ex(nullptr, n_nodes > 0 ? n_nodes : 1, n_sub).total;
}

int gtf_extract_candidates(const gtf_graph* g, const gtf_edges* e, const gtf_extract_io* io,
                           const gtf_extract_params* p, void* workspace, gtf_stream_t stream) {
    const char* who = "gtf_extract_candidates";
    if (int rc = gtf::check_abi(g, who)) return rc;
    if (!e || !io || !p || !workspace) return bad("gtf_extract_candidates: null argument");
    const int n = g->n_nodes;
    if (n <= 0) return 0;
    if (!io->xyzr || !io->vivl || !io->sub_id || !io->sub_ptr || !io->gnn || !io->label || !io->status ||
        !io->pval_xy || !io->pval_zr || !io->extracted || !io->n_candidates || p->fragment < 3)
        return bad("gtf_extract_candidates: missing arrays or fragment < 3");
    hipStream_t st = (hipStream_t)stream;
    const ExWs w = carve_ex(workspace, n, io->n_sub);
    const gtf::Cub cub{w.cub, st};
    hipError_t err;
    if (int rc = cca_rounds<false>(g, e, io->sub_id, io->n_sub, io->label, w.inactive, w.flag, st, who)) return rc;
    hipLaunchKernelGGL(k_ex_keys, dim3(grid(n)), dim3(BLOCK), 0, st, n, io->sub_id, io->sub_ptr, w.inactive,
                       io->order_key, io->label, w.keys_in, w.vals_in);
    if ((err = cub.sort_pairs(w.keys_in, w.keys_out, w.vals_in, w.vals_out, n)) != hipSuccess) return fail(who, "sort", err);
    hipLaunchKernelGGL(k_ex_starts, dim3(grid(n)), dim3(BLOCK), 0, st, n, w.keys_out, w.is_start);
    if ((err = cub.scan(w.is_start, w.cidx, n)) != hipSuccess) return fail(who, "scan", err);
    hipLaunchKernelGGL(k_ex_ptr, dim3(grid(n)), dim3(BLOCK), 0, st, n, w.is_start, w.cidx, w.cand_ptr,
                       io->n_candidates);
    hipLaunchKernelGGL(k_ex_candidate, dim3(grid(n)), dim3(BLOCK), 0, st, *io, *p, w.vals_out, w.cand_ptr,
                       io->n_candidates);
    hipLaunchKernelGGL(k_ex_flags, dim3(grid(n)), dim3(BLOCK), 0, st, n, *io);
    if ((err = hipGetLastError()) != hipSuccess) return fail(who, "launch", err);
    return 0;
}

}  // extern "C"
