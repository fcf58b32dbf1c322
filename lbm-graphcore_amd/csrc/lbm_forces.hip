// lbm_forces.hip -- momentum-exchange wall forces of the D2Q9 engine
// (include/lbm_forces_hip.h): the D2Q9 instantiation of the wall-list kernels
// (lbm_forces.hpp), the wall list itself (shared with the D3Q19 engine), and
// the engine's host side (list build from the ghosted obstacle map, totals,
// per-body sums, the planar map).
//
// An obstacle cell's stored populations are what the bounce-back of the last
// step left there (out_k = s_opp(k)), so the force is a function of the wall
// cell's own populations: a gather of at most eight floats per wall cell,
// gated by the link bits, in either lattice layout (the list holds offsets
// from the lattice origin) and on either ping-pong side.
//
// Arithmetic: IEEE fp32 in the written order, no contraction
// (-ffp-contract=off): the per-cell values equal lio.wall_force_cells of the
// stored cells bit for bit.

#include "lbm_forces.hpp"

#include <algorithm>
#include <climits>

#include "lbm_engine.hpp"
#include "lbm_forces_hip.h"

namespace lbm {
namespace forces {

namespace {

struct D2Q9 {
    static __device__ __forceinline__ void force(const float *p, long long ks, unsigned m, float &fx, float &fy,
                                                 float &fz) {
        float t[9];
#pragma unroll
        for (int j = 1; j < 9; ++j) t[j] = ((m >> (j - 1)) & 1u) ? p[j * ks] : 0.f;
        fx = ((t[3] + t[6] + t[7]) - (t[1] + t[5] + t[8])) * 2.f;
        fy = ((t[4] + t[7] + t[8]) - (t[2] + t[5] + t[6])) * 2.f;
        fz = 0.f;
    }
};

}  // namespace

hipError_t launch_wall2d(const WallArgs &a, int kind, hipStream_t s) { return launch_wall<D2Q9>(a, kind, s); }

// ---- the wall list (both engines) ----

void WallList::release() {
    for (void *p : {(void *)off, (void *)cell, (void *)mask, (void *)ctab, (void *)part, (void *)bpart})
        if (p) (void)hipFree(p);
    off = nullptr;
    cell = mask = ctab = nullptr;
    part = bpart = nullptr;
    nbodies = nc = nm = 0;
}

hipError_t WallList::upload(int nb) {
    release();
    n = (long long)h_off.size();
    if (n == 0) {
        nbodies = nb;
        return hipSuccess;
    }
#define WL_TRY(expr)                       \
    do {                                   \
        hipError_t e_ = (expr);            \
        if (e_ != hipSuccess) return e_;   \
    } while (0)
    const size_t un = (size_t)n;
    WL_TRY(hipMalloc(&off, sizeof(long long) * un));
    WL_TRY(hipMalloc(&cell, sizeof(unsigned) * un));
    WL_TRY(hipMalloc(&mask, sizeof(unsigned) * un));
    const size_t nblk = (size_t)wall_blocks(n);
    WL_TRY(hipMalloc(&part, (3 * sizeof(double) + sizeof(long long)) * nblk));
    if (nb <= 0) {
        WL_TRY(hipMemcpy(off, h_off.data(), sizeof(long long) * un, hipMemcpyHostToDevice));
        WL_TRY(hipMemcpy(cell, h_cell.data(), sizeof(unsigned) * un, hipMemcpyHostToDevice));
        WL_TRY(hipMemcpy(mask, h_mask.data(), sizeof(unsigned) * un, hipMemcpyHostToDevice));
        nbodies = 0;
        return hipSuccess;
    }
    // counting sort by body, stable: row-major inside a body, unlabelled cells last
    std::vector<unsigned> start((size_t)nb + 2, 0u);
    for (size_t i = 0; i < un; ++i) start[(size_t)(h_body[i] < 0 ? nb : h_body[i]) + 1]++;
    for (size_t b = 0; b <= (size_t)nb; ++b) start[b + 1] += start[b];
    std::vector<unsigned> at(start.begin(), start.end() - 1);
    std::vector<long long> s_off(un);
    std::vector<unsigned> s_cell(un), s_mask(un);
    for (size_t i = 0; i < un; ++i) {
        const unsigned d = at[(size_t)(h_body[i] < 0 ? nb : h_body[i])]++;
        s_off[d] = h_off[i];
        s_cell[d] = h_cell[i];
        s_mask[d] = h_mask[i];
    }
    WL_TRY(hipMemcpy(off, s_off.data(), sizeof(long long) * un, hipMemcpyHostToDevice));
    WL_TRY(hipMemcpy(cell, s_cell.data(), sizeof(unsigned) * un, hipMemcpyHostToDevice));
    WL_TRY(hipMemcpy(mask, s_mask.data(), sizeof(unsigned) * un, hipMemcpyHostToDevice));
    // chunks of at most BODY_CHUNK cells, body after body (the unlabelled tail has none)
    std::vector<unsigned> cs, cbody, mtab;
    for (size_t b = 0; b < (size_t)nb; ++b) {
        const unsigned s0 = start[b], s1 = start[b + 1];
        if (s0 == s1) continue;
        const unsigned first = (unsigned)cbody.size();
        const bool whole = s1 - s0 <= BODY_CHUNK;
        for (unsigned i = s0; i < s1; i += BODY_CHUNK) {
            cs.push_back(i);
            cbody.push_back((unsigned)b | (whole ? BODY_WHOLE : 0u));
        }
        if (!whole) mtab.insert(mtab.end(), {(unsigned)b, first, (unsigned)cbody.size()});
    }
    cs.push_back(start[(size_t)nb]);
    const size_t hnc = cbody.size();
    if (hnc > (size_t)INT_MAX) return hipErrorInvalidValue;
    std::vector<unsigned> tab(cs);
    tab.insert(tab.end(), cbody.begin(), cbody.end());
    tab.insert(tab.end(), mtab.begin(), mtab.end());
    WL_TRY(hipMalloc(&ctab, sizeof(unsigned) * tab.size()));
    WL_TRY(hipMemcpy(ctab, tab.data(), sizeof(unsigned) * tab.size(), hipMemcpyHostToDevice));
    WL_TRY(hipMalloc(&bpart, (3 * sizeof(double) + sizeof(long long)) * ((size_t)nb + hnc)));
    nbodies = nb;
    nc = (int)hnc;
    nm = (int)(mtab.size() / 3);
    return hipSuccess;
}

WallArgs WallList::args(const float *o, long long ks) const {
    WallArgs a{};
    a.o = o;
    a.ks = ks;
    a.off = off;
    a.mask = mask;
    a.cell = cell;
    a.n = n;
    a.part = part;
    a.lpart = part ? reinterpret_cast<long long *>(part + 3 * (size_t)wall_blocks(n)) : nullptr;
    a.nbodies = nbodies;
    if (bpart) {
        a.cs = ctab;
        a.cbody = ctab + nc + 1;
        a.mtab = a.cbody + nc;
        a.nc = nc;
        a.nm = nm;
        a.bsum = bpart;
        a.blinks = reinterpret_cast<long long *>(bpart + 3 * (size_t)nbodies);
        a.csum = reinterpret_cast<double *>(a.blinks + nbodies);
        a.clinks = reinterpret_cast<long long *>(a.csum + 3 * (size_t)nc);
    }
    return a;
}

hipError_t WallList::launch(int kind, const WallArgs &a, hipStream_t s) const {
    if (n == 0) return hipSuccess;  // nothing to gather: the outputs stay zero
    if (kind == WALL_BODIES) {      // a body without wall cells in this list has no chunk: its sums stay zero
        if (!bpart) return hipSuccess;
        const hipError_t e = hipMemsetAsync(bpart, 0, (3 * sizeof(double) + sizeof(long long)) * (size_t)nbodies, s);
        if (e != hipSuccess) return e;
    }
    return dims == 3 ? launch_wall3d(a, kind, s) : launch_wall2d(a, kind, s);
}

hipError_t WallList::fetch_total(hipStream_t s, double (&f)[3], long long &links) const {
    WL_TRY(hipStreamSynchronize(s));
    if (n == 0) return hipSuccess;
    const size_t nblk = (size_t)wall_blocks(n);
    std::vector<double> hp(4 * nblk);  // [nblk][3] doubles, then nblk long long
    WL_TRY(hipMemcpy(hp.data(), part, (3 * sizeof(double) + sizeof(long long)) * nblk, hipMemcpyDeviceToHost));
    std::vector<long long> hl(nblk);
    memcpy(hl.data(), hp.data() + 3 * nblk, sizeof(long long) * nblk);
    for (size_t b = 0; b < nblk; ++b) {  // block order
        for (int c = 0; c < 3; ++c) f[c] += hp[3 * b + c];
        links += hl[b];
    }
    return hipSuccess;
}

hipError_t WallList::fetch_bodies(hipStream_t s, double *fx, double *fy, double *fz, int64_t *links) const {
    WL_TRY(hipStreamSynchronize(s));
    if (n == 0 || nbodies <= 0) return hipSuccess;
    const size_t nb = (size_t)nbodies;
    std::vector<double> hp(4 * nb);
    WL_TRY(hipMemcpy(hp.data(), bpart, (3 * sizeof(double) + sizeof(long long)) * nb, hipMemcpyDeviceToHost));
    std::vector<long long> hl(nb);
    memcpy(hl.data(), hp.data() + 3 * nb, sizeof(long long) * nb);
    for (size_t b = 0; b < nb; ++b) {
        if (fx) fx[b] += hp[3 * b + 0];
        if (fy) fy[b] += hp[3 * b + 1];
        if (fz) fz[b] += hp[3 * b + 2];
        if (links) links[b] += hl[b];
    }
    return hipSuccess;
}
#undef WL_TRY

// what a handle that asked for forces holds: one list per local sub-domain
struct State {
    std::vector<WallList> lists;
    int nbodies = 0;  // bodies set (0: none)
};

}  // namespace forces
}  // namespace lbm

using lbm::forces::WallArgs;
using lbm::forces::WallList;

// ---- D2Q9 engine: host side ----

// the ghosted obstacle map of s (ring of og cells: periodic / neighbour images) back on the host
static std::vector<uint8_t> obst_g_host(const lbm_handle &h, const Sub &s) {
    std::vector<uint8_t> g((size_t)(s.w + 2 * h.og) * (s.h + 2 * h.og));
    HIP_CHECK(hipMemcpy(g.data(), s.obst_g, g.size(), hipMemcpyDeviceToHost));
    return g;
}

// Build the wall lists at the first force call: row-major per sub-domain; the
// links of a cell on a sub-domain border come from the ring of the ghosted
// map (the neighbour's cells, or the periodic image).
void lbm_handle::forces_build() {
    if (forces) return;
    auto *st = new lbm::forces::State();
    forces = st;  // owned by the handle from here (forces_release)
    st->lists.resize(subs.size());
    try {
        forces_fill();
    } catch (...) {
        forces_release();  // a later call builds again
        throw;
    }
}

void lbm_handle::forces_fill() {
    lbm::forces::State *st = forces;
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub &s = subs[k];
        set_device(s);
        if ((long long)s.w * s.h > (long long)INT_MAX) throw lbm_failure(LBM_E_INVALID, "sub-domain too large for a wall list");
        const std::vector<uint8_t> g = obst_g_host(*this, s);
        const int gw = s.w + 2 * og;
        WallList &wl = st->lists[k];
        wl.dims = 2;
        for (int y = 0; y < s.h; ++y) {
            const uint8_t *row = g.data() + (size_t)(y + og) * gw + og;
            for (int x = 0; x < s.w; ++x) {
                if (!row[x]) continue;
                unsigned m = 0;
                for (int j = 0; j < 8; ++j)
                    if (!row[x + DIR_Y[j] * gw + DIR_X[j]]) m |= 1u << j;
                if (m) wl.add((long long)y * s.pitch + x, (unsigned)((size_t)y * s.w + x), m);
            }
        }
        HIP_CHECK(wl.upload(0));
    }
}

void lbm_handle::forces_release() {
    if (!forces) return;
    for (size_t k = 0; k < forces->lists.size() && k < subs.size(); ++k)
        if (hipSetDevice(subs[k].dev) == hipSuccess) forces->lists[k].release();
    delete forces;
    forces = nullptr;
}

void lbm_handle::wall_force(double *fx, double *fy, int64_t *links) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take wall forces of");
    sync_all();
    forces_build();
    prof_drop();
    double f[3] = {0.0, 0.0, 0.0};
    long long nl = 0;
    for (size_t k = 0; k < subs.size(); ++k) {
        Sub &s = subs[k];
        set_device(s);
        const WallList &wl = forces->lists[k];
        const WallArgs a = wl.args(s.o[s.cur], s.plane);
        if (wl.n > 0)
            timed(s, s.s_comp, "wall_force", [&] { HIP_CHECK(wl.launch(lbm::forces::WALL_TOTAL, a, s.s_comp)); });
        HIP_CHECK(wl.fetch_total(s.s_comp, f, nl));  // sub-domain after sub-domain, blocks in order
    }
    prof_collect();
    if (fx) *fx = f[0];
    if (fy) *fy = f[1];
    if (links) *links = nl;
}

// Per-cell forces into planar host arrays float[ny][nx], each sub-domain at
// its rectangle: the wall cells scattered into zeroed staging arrays, then the
// copy of the fields path.
void lbm_handle::store_wall_force(float *fx, float *fy) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take wall forces of");
    if (!fx && !fy) return;
    sync_all();
    forces_build();
    prof_drop();
    float *const host[2] = {fx, fy};
    const int want = count_wanted(host, 2);
    for (size_t k = 0; k < subs.size(); ++k) {
        Sub &s = subs[k];
        set_device(s);
        const WallList &wl = forces->lists[k];
        WallArgs a = wl.args(s.o[s.cur], s.plane);
        const PlanarStage stage(want, (size_t)s.w * s.h);
        HIP_CHECK(hipMemsetAsync(stage.get(), 0, stage.bytes(), s.s_comp));
        float **dev[2] = {&a.mx, &a.my};
        for (int i = 0, n = 0; i < 2; ++i)
            if (host[i]) *dev[i] = stage.field(n++);
        if (wl.n > 0)
            timed(s, s.s_comp, "wall_force map", [&] { HIP_CHECK(wl.launch(lbm::forces::WALL_MAP, a, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        stage.copy_out(host, 2, host_span(s, false, 0), (size_t)s.w, (size_t)s.w, (size_t)s.h);
    }
    prof_collect();
}

void lbm_handle::set_bodies(const int32_t *labels, int32_t nbodies) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice: load cells before setting bodies");
    if ((labels && nbodies <= 0) || (!labels && nbodies != 0))
        throw lbm_failure(LBM_E_INVALID, "labels with nbodies <= 0, or NULL labels with nbodies != 0");
    sync_all();
    forces_build();
    if (!labels) {
        if (forces->nbodies == 0) return;
        for (size_t k = 0; k < subs.size(); ++k) {
            set_device(subs[k]);
            forces->lists[k].h_body.clear();
            HIP_CHECK(forces->lists[k].upload(0));
        }
        forces->nbodies = 0;
        return;
    }
    // every blocked cell's label is checked before anything changes
    std::vector<std::vector<int>> body(subs.size());
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub &s = subs[k];
        set_device(s);
        const std::vector<uint8_t> g = obst_g_host(*this, s);
        const int gw = s.w + 2 * og;
        for (int y = 0; y < s.h; ++y)
            for (int x = 0; x < s.w; ++x)
                if (g[(size_t)(y + og) * gw + og + x] && labels[(size_t)(s.rect.y0 + y) * p.nx + s.rect.x0 + x] >= nbodies)
                    throw lbm_failure(LBM_E_INVALID, "label >= nbodies on a blocked cell");
        const WallList &wl = forces->lists[k];
        body[k].resize(wl.h_cell.size());
        for (size_t i = 0; i < wl.h_cell.size(); ++i) {
            const int y = (int)(wl.h_cell[i] / (unsigned)s.w), x = (int)(wl.h_cell[i] % (unsigned)s.w);
            const int32_t l = labels[(size_t)(s.rect.y0 + y) * p.nx + s.rect.x0 + x];
            body[k][i] = l < 0 ? -1 : l;
        }
    }
    for (size_t k = 0; k < subs.size(); ++k) {
        set_device(subs[k]);
        forces->lists[k].h_body.swap(body[k]);
        HIP_CHECK(forces->lists[k].upload(nbodies));
    }
    forces->nbodies = nbodies;
}

void lbm_handle::body_forces(double *fx, double *fy, int64_t *links, int32_t nbodies) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take wall forces of");
    if (!forces || forces->nbodies == 0 || forces->nbodies != nbodies)
        throw lbm_failure(LBM_E_STATE, "lbm_body_forces: no bodies set, or set with another nbodies");
    sync_all();
    prof_drop();
    for (int b = 0; b < nbodies; ++b) {
        if (fx) fx[b] = 0.0;
        if (fy) fy[b] = 0.0;
        if (links) links[b] = 0;
    }
    for (size_t k = 0; k < subs.size(); ++k) {
        Sub &s = subs[k];
        set_device(s);
        const WallList &wl = forces->lists[k];
        const WallArgs a = wl.args(s.o[s.cur], s.plane);
        if (wl.n > 0)
            timed(s, s.s_comp, "wall_force bodies",
                  [&] { HIP_CHECK(wl.launch(lbm::forces::WALL_BODIES, a, s.s_comp)); });
        HIP_CHECK(wl.fetch_bodies(s.s_comp, fx, fy, nullptr, links));  // sub-domain after sub-domain
    }
    prof_collect();
}
