// lbm3d_engine.hip -- run path of the D3Q19 engine (lbm3d_engine.hpp): create,
// tuning knobs, allocation, placement probe, the step loop (one step per
// launch, two or three steps per pass), ghost exchange over RCCL or device
// copies, load / store / destroy.  Kernels and lattice layout: lbm3d.hip.

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lbm3d_engine.hpp"

using namespace lbm;

// tuning knobs only with LBM_DEBUG_KNOBS=1 (as the 2-D engine); LBM_POISON always
void lbm3d_handle::read_tuning() {
    const char *dk = getenv("LBM_DEBUG_KNOBS");
    const bool knobs = dk && *dk && atoi(dk) != 0;
    const char *po = getenv("LBM_POISON");
    poison = po && *po && atoi(po) != 0;
    auto knob = [&](const char *name) -> const char * {
        const char *v = knobs ? getenv(name) : nullptr;
        return (v && *v) ? v : nullptr;
    };
    const char *pe = knob("LBM3D_PAIR");
    pair = p.nx % 2 == 0 && !(pe && atoi(pe) == 0);
    if (const char *z = knob("LBM3D_ZB")) zb = (atoi(z) == 1 || atoi(z) == 4 || atoi(z) == 8) ? atoi(z) : 2;
    if (const char *n = knob("LBM3D_NT")) nt = atoi(n) != 0;
    if (const char *t = knob("LBM3D_TWO")) two = atoi(t) != 0;
    if (const char *g = knob("LBM3D_SEG")) seg = std::max(1, atoi(g));
    if (const char *t = knob("LBM3D_THREE")) three = atoi(t) != 0 ? 1 : 0;
    if (const char *g = knob("LBM3D_SEG3")) seg3 = std::max(1, atoi(g));
    if (const char *h = knob("LBM3D_TH")) th = atoi(h);
    if (const char *k = knob("LBM3D_SKIP")) skip = atoi(k) != 0;
    if (const char *k = knob("LBM3D_SKIP3")) skip3 = atoi(k) != 0;
    if (const char *d = knob("LBM3D_PD")) pd = atoi(d);
    if (const char *k = knob("LBM3D_KSPAD")) kspad = (std::max(0LL, atoll(k)) + 63) / 64 * 64;
    lattice_pad = knob("LBM_LATTICE_PAD");
    if (const char *t = knob("LBM3D_PLACEMENT_TRIES")) probe_tries = std::max(1, atoi(t));
    if (const char *m = knob("LBM3D_PROBE_MIN_CELLS")) probe_min_cells = std::max(0LL, atoll(m));
    if (const char *pt = knob("LBM3D_PROBE_THREE")) probe_three = atoi(pt) != 0;
    probe_log = knob("LBM_PLACEMENT_LOG") != nullptr;
    if (const char *d = knob("LBM_DEBUG_DELAY_SUB")) delay_sub = atoi(d);
    if (const char *d = knob("LBM_DEBUG_DELAY_US")) delay_us = std::min(std::max(atoi(d), 0), 100000);
    if (tolerance) {  // the tolerance pass exists for the default block only
        th = 12;
        skip = false;
        pd = 0;
    }
    // the two-step kernel is instantiated for these (rows, skip, prefetch)
    // combinations only; anything else is rejected here, never launched as
    // a different template (blocks of 64 x th threads, at most 960)
    if (two_variant(th, skip, pd) < 0)
        throw lbm_failure(LBM_E_INVALID, "unsupported two-step block: LBM3D_TH " + std::to_string(th) + ", SKIP " +
                                             std::to_string(skip ? 1 : 0) + ", PD " + std::to_string(pd));
}

void lbm3d_handle::create(const lbm3d_params *prm, const uint8_t *obstacles, const lbm_config &cfg) {
    p = *prm;
    if (p.nx <= 0 || p.ny <= 0 || p.nz <= 0 || p.max_iters < 0)
        throw lbm_failure(LBM_E_INVALID, "nx, ny, nz must be > 0 and max_iters >= 0");
    if (!obstacles) throw lbm_failure(LBM_E_INVALID, "obstacles must not be NULL");
    parts = cfg.parts > 0 ? cfg.parts : 1;
    transport = cfg.transport;
    tolerance = (cfg.flags & LBM_FLAG_TOLERANCE) != 0;
    if (parts > p.nz) throw lbm_failure(LBM_E_INVALID, "more z slabs than planes");
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw lbm_failure(LBM_E_HIP, "no HIP device visible");
    const long long cells = (long long)p.nx * p.ny * p.nz;
    free_cells = 0;
    for (long long i = 0; i < cells; ++i) free_cells += obstacles[i] ? 0 : 1;
    px = (p.nx + 15) / 16 * 16;  // 64-byte rows
    read_tuning();
    KS = (long long)p.ny * px + kspad;
    PL = (long long)Q3 * KS;
    // round-robin z extents (StructuredGridUtils.hpp:161-165 rule, in z)
    all_z0.assign(parts, 0);
    all_nz.assign(parts, p.nz / parts);
    for (int i = 0; i < p.nz % parts; ++i) all_nz[i]++;
    for (int i = 1; i < parts; ++i) all_z0[i] = all_z0[i - 1] + all_nz[i - 1];
    std::vector<int> mine;
    if (transport == LBM_TRANSPORT_RCCL) {
        if (cfg.world != parts || cfg.rank < 0 || cfg.rank >= parts)
            throw lbm_failure(LBM_E_INVALID, "RCCL transport needs world == parts and 0 <= rank < world");
        if (!cfg.rccl_unique_id) throw lbm_failure(LBM_E_INVALID, "RCCL transport needs rccl_unique_id");
        rank = cfg.rank;
        world = cfg.world;
        mine.push_back(rank);
    } else if (transport == LBM_TRANSPORT_LOCAL) {
        for (int i = 0; i < parts; ++i) mine.push_back(i);
    } else {
        throw lbm_failure(LBM_E_INVALID, "unknown transport");
    }
    slabs.resize(mine.size());
    for (size_t k = 0; k < mine.size(); ++k) {
        Slab &s = slabs[k];
        s.id = mine[k];
        s.z0 = all_z0[s.id];
        s.nzs = all_nz[s.id];
        if (transport == LBM_TRANSPORT_RCCL)
            s.dev = (cfg.devices && cfg.num_devices > 0) ? cfg.devices[0] : rank % ndev;
        else
            s.dev = (cfg.devices && cfg.num_devices > 0) ? cfg.devices[s.id % cfg.num_devices] : s.id % ndev;
        if (s.dev < 0 || s.dev >= ndev) throw lbm_failure(LBM_E_INVALID, "device index out of range");
        alloc(s, obstacles);
    }
    if (transport == LBM_TRANSPORT_RCCL) {
        ncclUniqueId id;
        memcpy(&id, cfg.rccl_unique_id, sizeof(id));
        HIP_CHECK(hipSetDevice(slabs[0].dev));
        NCCL_CHECK(ncclCommInitRank(&comm, world, id, rank));
    } else if (slabs.size() > 1) {
        for (auto &a : slabs)
            for (auto &b : slabs)
                if (a.dev != b.dev) {
                    int can = 0;
                    HIP_CHECK(hipDeviceCanAccessPeer(&can, a.dev, b.dev));
                    if (can) {
                        HIP_CHECK(hipSetDevice(a.dev));
                        hipError_t e = hipDeviceEnablePeerAccess(b.dev, 0);
                        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_CHECK(e);
                        (void)hipGetLastError();
                    }
                }
    }
    ensure_av(std::max(p.max_iters, 1));
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    HIP_CHECK(hipEventCreate(&t0));
    HIP_CHECK(hipEventCreate(&t1));
    placement_probe();
}

// Placement probe (the D3Q19 counterpart of lbm_engine.hip's; DESIGN.md
// §4.9): the two-step pass runs at an engine-to-engine spread of about
// +-5 % at 512^3 fixed by where the lattices land (39.9-44.2 GLUPS over
// six engines in one process, profiles/r03/d3q19/spread.log).  A single
// slab of at least 2^26 cells allocates up to probe_tries lattice pairs
// (at most 128 GB held at once: six at 512^3), times the engine's passes
// on each (constant populations; one warm-up round, then the best of two
// interleaved rounds), keeps the fastest pair and frees the rest; the kept
// pair is filled as a fresh allocation is, so the engine's state is as if
// the probe had not run.  Failures inside free every extra candidate and
// restore the original pair.
// Scope: single-slab engines; each candidate is timed with the engine's
// own pass form (three-step passes, the default in both numerics since
// round 4, or two-step ones).  Round 4 first timed two-step passes for
// three-step engines and gained nothing (profiles/r04/prof1/d3_probe.log);
// timing their own three-step passes it keeps the fast placement
// (7.1-7.2 vs 7.4-7.8 ms per tolerance pass): 55.0-55.9 GLUPS over four
// engines against 51.5-55.4 unprobed (profiles/r04/d3q19/ab_probe3.log).
// LBM3D_PROBE_THREE=0 skips the probe for three-step engines (A/B).
void lbm3d_handle::placement_probe() {
    if (multi() || !use_two() || (use_three() && !probe_three) || slabs.size() != 1) return;
    Slab &s = slabs[0];
    if ((long long)p.nx * p.ny * p.nz < probe_min_cells || s.f_joint) return;
    const size_t floats = (size_t)(s.nzs + 2 * GZ3) * PL;
    const size_t pair_bytes = 2 * sizeof(float) * floats;
    const int cap = (int)std::max<size_t>(1, (128ull << 30) / pair_bytes);
    const int tries = std::min({probe_tries, 8, cap});
    if (tries <= 1) return;
    HIP_CHECK(hipSetDevice(s.dev));
    std::vector<std::array<float *, 2>> cand{{s.f[0], s.f[1]}};
    size_t keep = 0;
    auto set_pair = [&](size_t c) {
        for (int k = 0; k < 2; ++k) {
            s.f[k] = cand[c][k];
            s.o[k] = s.f[k] + GZ3 * PL;
        }
        s.cur = 0;
    };
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const int depth = use_three() ? 3 : 2;  // the engine's own pass form
    try {
        for (int c = 1; c < tries; ++c) {
            std::array<float *, 2> f{nullptr, nullptr};
            if (hipMalloc(&f[0], sizeof(float) * floats) != hipSuccess) { (void)hipGetLastError(); break; }
            if (hipMalloc(&f[1], sizeof(float) * floats) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipFree(f[0]);
                break;
            }
            cand.push_back(f);
        }
        for (auto &f : cand)  // 0.05f everywhere: rho = 0.95, no tiny-density path
            for (float *q : f)
                HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(q), 0x3d4ccccd, floats, s.s_comp));
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        std::vector<float> best(cand.size(), 1e30f);
        for (int round = 0; round < 3; ++round)
            for (size_t c = 0; c < cand.size(); ++c) {
                set_pair(c);
                HIP_CHECK(hipEventRecord(e0, s.s_comp));
                for (int i = 0; i < 2; ++i) {
                    launch_pass(depth, s, 0, s.nzs, 0, s.s_comp);
                    s.cur ^= 1;
                }
                HIP_CHECK(hipEventRecord(e1, s.s_comp));
                HIP_CHECK(hipEventSynchronize(e1));
                float ms = 0.f;
                HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (round > 0) best[c] = std::min(best[c], ms / 2);  // round 0: clock warm-up
            }
        for (size_t c = 1; c < cand.size(); ++c)
            if (best[c] < best[keep]) keep = c;
        if (probe_log) {
            fprintf(stderr, "lbm3d placement probe (%dx%dx%d): ms per %s-step pass", p.nx, p.ny, p.nz,
                    depth == 3 ? "three" : "two");
            for (float v : best) fprintf(stderr, " %.4f", v);
            fprintf(stderr, "; kept pair %zu\n", keep);
        }
        for (size_t c = 0; c < cand.size(); ++c)
            if (c != keep)
                for (float *&q : cand[c]) {
                    (void)hipFree(q);
                    q = nullptr;
                }
        set_pair(keep);
        for (float *q : s.f) fill_fresh(q, sizeof(float) * floats, s.s_comp);
        HIP_CHECK(hipEventDestroy(e0));
        HIP_CHECK(hipEventDestroy(e1));
    } catch (...) {
        // the handle keeps exactly one pair: the original while it exists, else the kept one
        const size_t own = cand[0][0] ? 0 : keep;
        for (size_t c = 0; c < cand.size(); ++c)
            if (c != own)
                for (float *&q : cand[c])
                    if (q) {
                        (void)hipFree(q);
                        q = nullptr;
                    }
        set_pair(own);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        throw;
    }
}

void lbm3d_handle::alloc(Slab &s, const uint8_t *obstacles) {
    HIP_CHECK(hipSetDevice(s.dev));
    // streams first: every initial fill below is ordered on s_comp (a
    // null-stream hipMemset is not ordered with these non-blocking streams)
    HIP_CHECK(hipStreamCreateWithFlags(&s.s_comp, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&s.s_comm, hipStreamNonBlocking));
    int lo = 0, hi = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_CHECK(hipStreamCreateWithPriority(&s.s_bnd, hipStreamNonBlocking, hi));
    for (hipEvent_t *e : {&s.ev_b, &s.ev_i, &s.ev_x, &s.ev_end})
        HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    // three ghost planes below and above (the three-step kernel reads all of them)
    const size_t floats = (size_t)(s.nzs + 2 * GZ3) * PL;
    const char *lp = lattice_pad;
    if (lp && *lp) {
        // both lattices in one allocation, the second pad bytes (rounded to
        // 256 B) after the end of the first (see lbm_engine.hip alloc_sub)
        const size_t second = floats + (size_t)(std::max(0LL, atoll(lp)) + 255) / 256 * 64;
        const size_t n = (second + floats) * sizeof(float);
        HIP_CHECK(hipMalloc(&s.f[0], n));
        fill_fresh(s.f[0], n, s.s_comp);
        s.f[1] = s.f[0] + second;
        s.f_joint = true;
    } else {
        for (int k = 0; k < 2; ++k) {
            HIP_CHECK(hipMalloc(&s.f[k], floats * sizeof(float)));
            fill_fresh(s.f[k], floats * sizeof(float), s.s_comp);
        }
    }
    for (int k = 0; k < 2; ++k) s.o[k] = s.f[k] + GZ3 * PL;
    const size_t ob = (size_t)s.nzs * p.ny * p.nx, plane = (size_t)p.ny * p.nx;
    HIP_CHECK(hipMalloc(&s.obst, ob + 256));
    HIP_CHECK(hipMemcpy(s.obst, obstacles + (size_t)s.z0 * plane, ob, hipMemcpyHostToDevice));
    HIP_CHECK(hipMalloc(&s.obst_g, (size_t)(s.nzs + 2 * GZ3) * plane + 256));
    for (int z = -GZ3; z < s.nzs + GZ3; ++z) {  // global periodic images (the neighbour slabs' planes)
        const int gz = ((s.z0 + z) % p.nz + p.nz) % p.nz;
        HIP_CHECK(hipMemcpy(s.obst_g + (size_t)(z + GZ3) * plane, obstacles + (size_t)gz * plane, plane,
                            hipMemcpyHostToDevice));
    }
    // multi: two one-plane boundary launches, then the interior launch
    s.nblk_bnd = multi() ? (s.nzs >= 2 ? 2 : 1) * blocks_for(1) : 0;
    s.nblk_int = multi() ? blocks_for(s.nzs - 2) : 0;
    s.nblk_all = multi() ? s.nblk_bnd + s.nblk_int : blocks_for(s.nzs);
    HIP_CHECK(hipMalloc(&s.partials, sizeof(float) * (size_t)(s.nblk_all + 64)));
    fill_fresh(s.partials, sizeof(float) * (size_t)(s.nblk_all + 64), s.s_comp);
    for (int n = 2; n <= 3; ++n) {  // every slab has at least one plane: a pass has at least one block
        int &nblk = s.pass_nblk[n - 2];
        nblk = 0;
        for (const auto &r : pass_ranges(n, s)) nblk += pass_blocks(n, r.first, r.second);
        const size_t bytes = sizeof(float) * ((size_t)n * nblk + 64);
        HIP_CHECK(hipMalloc(&s.pass_partials[n - 2], bytes));
        fill_fresh(s.pass_partials[n - 2], bytes, s.s_comp);
    }
}

// Initial fill of a fresh allocation on `st`, waited for: zero, or with
// LBM_POISON=1 all-ones bytes (NaN floats) -- a read of anything the
// engine did not write then shows up as NaN (tests/test_poison.py).
void lbm3d_handle::fill_fresh(void *ptr, size_t bytes, hipStream_t st) const {
    HIP_CHECK(hipMemsetAsync(ptr, poison ? 0xFF : 0, bytes, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

// ---- n-step passes (n = 2: step3d_two, n = 3: step3d_three) ----

// Two-step passes (LBM3D_TWO): one slab, or z slabs of at least 4 planes;
// three-step passes (LBM3D_THREE, needs two): one slab, or z slabs of at least
// 6 planes -- the ghosts are n planes of the neighbours, exchanged once per pass.
bool lbm3d_handle::use_pass(int n) const {
    if (!two) return false;
    // step3d_three addresses a plane's speeds by 32-bit buffer offsets
    if (n == 3 && (three == 0 || !use_pass(2) || (long long)Q3 * KS * 4 >= (1LL << 31))) return false;
    if (multi())
        for (int nz : all_nz)
            if (nz < 2 * n) return false;
    return true;
}

// Output plane ranges of one n-step pass of slab s, in launch order.
// Single slab: all planes.  z slabs: the two boundary ranges [0, n) and
// [nzs-n, nzs) first (their outputs are the next pass's exchanged ghost
// planes), then the interior [n, nzs-n), which reads no ghost plane and
// runs while the exchange moves.
std::vector<std::pair<int, int>> lbm3d_handle::pass_ranges(int n, const Slab &s) const {
    if (!multi() || s.nzs < 2 * n) return {{0, s.nzs}};
    std::vector<std::pair<int, int>> r = {{0, n}, {s.nzs - n, s.nzs}};
    if (s.nzs > 2 * n) r.push_back({n, s.nzs - n});
    return r;
}


// output planes [z0, zn) of slab s, partials from block blk0 of the pass
void lbm3d_handle::launch_pass(int n, Slab &s, int z0, int zn, int blk0, hipStream_t st) {
    const Two3Args a{s.o[s.cur], s.o[1 - s.cur], s.obst_g + (size_t)GZ3 * p.ny * p.nx,  // fin, fout, obst
                     PL, KS, px, p.nx, p.ny, s.nzs, pass_seg(n), z0, zn,
                     p.omega, 1 - p.omega, w1(), w2(),                                    // omega, omo, w1, w2
                     p.omega * (1.f / 3.f), p.omega * (1.f / 18.f), p.omega * (1.f / 36.f),  // k0, k1, k2
                     s.pass_partials[n - 2], s.pass_nblk[n - 2], blk0};
    if (n == 3)
        HIP_CHECK(launch_step3d_three(a, tolerance, skip3, st));
    else
        HIP_CHECK(launch_step3d_two(a, two_variant(th, skip, pd), tolerance, st));
}

// the pass's n steps' |u|
void lbm3d_handle::reduce_pass(int n, Slab &s, int t, hipStream_t st) {
    const int nblk = s.pass_nblk[n - 2];
    for (int l = 0; l < n; ++l)
        HIP_CHECK(launch_reduce3d(s.pass_partials[n - 2] + (size_t)l * nblk, nblk, s.av_local, t + l, st));
}

// n steps of every slab (z slabs): B(t) = the boundary ranges on the
// high-priority stream after I(t-1) and the exchange that filled our
// ghosts; X(t) = their planes to the neighbours on the comm stream; I(t) =
// the interior on the compute stream, overlapping X(t); then the n steps'
// |u| folds.  (Mirrors step_once's one-plane schedule.)
void lbm3d_handle::step_pass_multi(int n, int t) {
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipStreamWaitEvent(s.s_bnd, s.ev_i, 0));
        wait_x(s, s.s_bnd);
        stall(s, s.s_bnd);
        const auto r = pass_ranges(n, s);
        int blk = 0;
        for (size_t i = 0; i < r.size() && i < 2; ++i) {
            launch_pass(n, s, r[i].first, r[i].second, blk, s.s_bnd);
            blk += pass_blocks(n, r[i].first, r[i].second);
        }
        HIP_CHECK(hipEventRecord(s.ev_b, s.s_bnd));
    }
    post_exchange(1 - slabs[0].cur, n, true);
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        const auto r = pass_ranges(n, s);
        stall(s, s.s_comp);
        if (r.size() > 2)
            launch_pass(n, s, r[2].first, r[2].second,
                        pass_blocks(n, r[0].first, r[0].second) + pass_blocks(n, r[1].first, r[1].second), s.s_comp);
        HIP_CHECK(hipStreamWaitEvent(s.s_comp, s.ev_b, 0));
        reduce_pass(n, s, t, s.s_comp);
        HIP_CHECK(hipEventRecord(s.ev_i, s.s_comp));
        s.cur ^= 1;
    }
}

// n-step pass; single slab: ghost planes -n .. -1, nz .. nz + n - 1 of the
// current lattice (periodic images, all 19 speeds), the pass kernel, then
// the n steps' |u|
void lbm3d_handle::step_pass(int n, int t) {
    if (multi()) {
        step_pass_multi(n, t);
        return;
    }
    Slab &s = slabs[0];
    const size_t bytes = sizeof(float) * (size_t)PL;
    float *o = s.o[s.cur];
    for (int i = -n; i < n; ++i) {
        const int g = i < 0 ? i : s.nzs + i, src = ((g % s.nzs) + s.nzs) % s.nzs;
        HIP_CHECK(hipMemcpyAsync(o + (long long)g * PL, o + (long long)src * PL, bytes, hipMemcpyDeviceToDevice,
                                 s.s_comp));
    }
    launch_pass(n, s, 0, s.nzs, 0, s.s_comp);
    reduce_pass(n, s, t, s.s_comp);
    s.cur ^= 1;
    exchange(s.cur, false);  // faces for a one-step launch that may follow
}

void lbm3d_handle::ensure_av(int n) {
    for (auto &s : slabs) {
        if (s.av_cap >= n) continue;
        HIP_CHECK(hipSetDevice(s.dev));
        if (s.av_local) HIP_CHECK(hipFree(s.av_local));
        s.av_cap = std::max(n, 1);
        HIP_CHECK(hipMalloc(&s.av_local, sizeof(float) * (size_t)s.av_cap));
        fill_fresh(s.av_local, sizeof(float) * (size_t)s.av_cap, s.s_comp);
    }
}

Slab *lbm3d_handle::local(int id) {
    for (auto &s : slabs)
        if (s.id == id) return &s;
    return nullptr;
}

// ---- ghost exchange ----

// n = 1 (one-step launches): one contiguous face block per message -- speeds
// 9..13 of the top plane go up, 14..18 of the bottom plane go down, into the
// same speeds of the neighbours' inner ghost planes.  n = 2, 3 (n-step
// passes): all 19 speeds of n planes -- planes nzs-n .. nzs-1 go up into the
// next slab's ghosts -n .. -1; planes 0 .. n-1 go down into the previous
// slab's ghosts nzs .. nzs+n-1.
Ends3 lbm3d_handle::ends(const Slab &s, int n) const {
    if (n == 1) return {(s.nzs - 1) * PL + 9 * KS, 14 * KS, -PL + 9 * KS, s.nzs * PL + 14 * KS, 5 * KS};
    return {(s.nzs - n) * PL, 0, -n * PL, s.nzs * PL, n * PL};
}

// Post the exchange of ends(., n) of lattice l of every slab, on its comm or
// compute stream after event ev_b of the source slabs.  Every rank posts send
// up, send down, recv from below, recv from above (RCCL matches by order).
void lbm3d_handle::post_exchange(int l, int n, bool use_comm) {
    if (transport == LBM_TRANSPORT_RCCL) {
        Slab &s = slabs[0];
        const Ends3 e = ends(s, n);
        HIP_CHECK(hipSetDevice(s.dev));
        hipStream_t st = use_comm ? s.s_comm : s.s_comp;
        HIP_CHECK(hipStreamWaitEvent(st, s.ev_b, 0));
        NCCL_CHECK(ncclGroupStart());
        for (const lbm_xfer &x : slab_posts(rank, world, e.floats)) {
            if (x.op == LBM_XFER_SEND)
                NCCL_CHECK(ncclSend(s.o[l] + (x.dir == 0 ? e.up_src : e.down_src), (size_t)x.floats, ncclFloat, x.peer,
                                    comm, st));
            else
                NCCL_CHECK(ncclRecv(s.o[l] + (x.dir == 1 ? e.ghost_lo : e.ghost_hi), (size_t)x.floats, ncclFloat,
                                    x.peer, comm, st));
        }
        NCCL_CHECK(ncclGroupEnd());
        HIP_CHECK(hipEventRecord(s.ev_x, st));
        return;
    }
    for (auto &s : slabs) {  // LOCAL: each slab pulls its two ghost blocks
        HIP_CHECK(hipSetDevice(s.dev));
        hipStream_t st = use_comm ? s.s_comm : s.s_comp;
        Slab *below = local((s.id + parts - 1) % parts), *above = local((s.id + 1) % parts);
        HIP_CHECK(hipStreamWaitEvent(st, below->ev_b, 0));
        HIP_CHECK(hipStreamWaitEvent(st, above->ev_b, 0));
        const Ends3 e = ends(s, n);
        const size_t bytes = sizeof(float) * (size_t)e.floats;
        float *lo = s.o[l] + e.ghost_lo, *hi = s.o[l] + e.ghost_hi;
        const float *from_below = below->o[l] + ends(*below, n).up_src, *from_above = above->o[l] + ends(*above, n).down_src;
        if (below->dev == s.dev)
            HIP_CHECK(hipMemcpyAsync(lo, from_below, bytes, hipMemcpyDeviceToDevice, st));
        else
            HIP_CHECK(hipMemcpyPeerAsync(lo, s.dev, from_below, below->dev, bytes, st));
        if (above->dev == s.dev)
            HIP_CHECK(hipMemcpyAsync(hi, from_above, bytes, hipMemcpyDeviceToDevice, st));
        else
            HIP_CHECK(hipMemcpyPeerAsync(hi, s.dev, from_above, above->dev, bytes, st));
        HIP_CHECK(hipEventRecord(s.ev_x, st));
    }
}

// Fill the inner ghost planes' face speeds of lattice l of every slab.
// Single slab: periodic self copies.
void lbm3d_handle::exchange(int l, bool use_comm) {
    if (multi()) {
        post_exchange(l, 1, use_comm);
        return;
    }
    Slab &s = slabs[0];
    const Ends3 e = ends(s, 1);
    const size_t bytes = sizeof(float) * (size_t)e.floats;
    HIP_CHECK(hipSetDevice(s.dev));
    HIP_CHECK(hipMemcpyAsync(s.o[l] + e.ghost_lo, s.o[l] + e.up_src, bytes, hipMemcpyDeviceToDevice, s.s_comp));
    HIP_CHECK(hipMemcpyAsync(s.o[l] + e.ghost_hi, s.o[l] + e.down_src, bytes, hipMemcpyDeviceToDevice, s.s_comp));
}

void lbm3d_handle::stall(const Slab &s, hipStream_t st) {
    if (delay_us > 0 && s.id == delay_sub) HIP_CHECK(launch_debug_spin(delay_us, st));
}

// st waits for this slab's last exchange and (LOCAL) its neighbours' (they read our faces)
void lbm3d_handle::wait_x(Slab &s, hipStream_t st) {
    HIP_CHECK(hipStreamWaitEvent(st, s.ev_x, 0));
    if (transport == LBM_TRANSPORT_LOCAL && multi()) {
        HIP_CHECK(hipStreamWaitEvent(st, local((s.id + parts - 1) % parts)->ev_x, 0));
        HIP_CHECK(hipStreamWaitEvent(st, local((s.id + 1) % parts)->ev_x, 0));
    }
}

// ---- one step per launch ----

void lbm3d_handle::launch(Slab &s, int zfirst, int planes, float *partials, hipStream_t st) {
    const Step3Args a{s.o[s.cur], s.o[1 - s.cur], s.obst + (size_t)zfirst * p.ny * p.nx,  // fin, fout, obst
                      PL, KS, px, p.nx, p.ny, zfirst, p.omega, 1 - p.omega, w1(), w2(), partials};
    HIP_CHECK(launch_step3d(a, planes, pair, zb, nt, st));
}

// one step of every slab: reads lattice cur, writes 1 - cur and its ghosts
void lbm3d_handle::step_once(int t) {
    if (!multi()) {
        Slab &s = slabs[0];
        launch(s, 0, s.nzs, s.partials, s.s_comp);
        exchange(1 - s.cur, false);
        HIP_CHECK(launch_reduce3d(s.partials, s.nblk_all, s.av_local, t, s.s_comp));
        s.cur ^= 1;
        return;
    }
    // B(t): faces, after I(t-1) and the exchanges that filled / read our ghosts and faces
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipStreamWaitEvent(s.s_bnd, s.ev_i, 0));
        wait_x(s, s.s_bnd);
        stall(s, s.s_bnd);
        launch(s, 0, 1, s.partials, s.s_bnd);
        if (s.nzs >= 2) launch(s, s.nzs - 1, 1, s.partials + blocks_for(1), s.s_bnd);
        HIP_CHECK(hipEventRecord(s.ev_b, s.s_bnd));
    }
    // X(t): faces of the new lattice -> neighbours' ghost planes, on the comm streams
    exchange(1 - slabs[0].cur, true);
    // I(t): interior planes, after B(t) (reduction needs its partials; the
    // interior reads the faces B(t-1) wrote, already ordered by ev_b)
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        stall(s, s.s_comp);
        launch(s, 1, s.nzs - 2, s.partials + s.nblk_bnd, s.s_comp);
        HIP_CHECK(hipStreamWaitEvent(s.s_comp, s.ev_b, 0));
        HIP_CHECK(launch_reduce3d(s.partials, s.nblk_all, s.av_local, t, s.s_comp));
        HIP_CHECK(hipEventRecord(s.ev_i, s.s_comp));
        s.cur ^= 1;
    }
}

void lbm3d_handle::sync_all() {
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_bnd));
        HIP_CHECK(hipStreamSynchronize(s.s_comm));
    }
}

// ghost planes of the current lattice, from its faces (after load / init)
void lbm3d_handle::refresh() {
    if (multi())
        for (auto &s : slabs) {
            HIP_CHECK(hipSetDevice(s.dev));
            HIP_CHECK(hipEventRecord(s.ev_b, s.s_comp));
        }
    exchange(slabs[0].cur, false);
    sync_all();
}

void lbm3d_handle::run_steps(int steps) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "lattice not initialised (lbm3d_load_cells / lbm3d_init_equilibrium)");
    if (steps < 0) throw lbm_failure(LBM_E_INVALID, "steps must be >= 0");
    ensure_av(std::max(steps, 1));
    sync_all();
    Slab &s0 = slabs[0];
    HIP_CHECK(hipSetDevice(s0.dev));
    HIP_CHECK(hipEventRecord(t0, s0.s_comp));
    for (auto &s : slabs) {  // every stream starts after t0 and the last refresh
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipStreamWaitEvent(s.s_comp, t0, 0));
        HIP_CHECK(hipEventRecord(s.ev_i, s.s_comp));
        HIP_CHECK(hipEventRecord(s.ev_x, s.s_comp));
    }
    int t = 0;
    run_three = run_two = run_one = 0;
    if (use_two() && steps >= 2) {
        if (multi()) {  // two- / three-plane ghosts of the current lattice (a one-step launch leaves only its five speeds)
            for (auto &s : slabs) {
                HIP_CHECK(hipSetDevice(s.dev));
                HIP_CHECK(hipEventRecord(s.ev_b, s.s_comp));
            }
            post_exchange(slabs[0].cur, use_three() && steps >= 3 ? 3 : 2, false);
        }
        if (use_three())
            for (; t + 3 <= steps; t += 3, ++run_three) step_pass(3, t);
        for (; t + 2 <= steps; t += 2, ++run_two) step_pass(2, t);
    }
    for (; t < steps; ++t, ++run_one) step_once(t);
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipStreamWaitEvent(s.s_comp, s.ev_x, 0));
        HIP_CHECK(hipEventRecord(s.ev_end, s.s_comp));
    }
    HIP_CHECK(hipSetDevice(s0.dev));
    for (auto &s : slabs) HIP_CHECK(hipStreamWaitEvent(s0.s_comp, s.ev_end, 0));
    HIP_CHECK(hipEventRecord(t1, s0.s_comp));
    HIP_CHECK(hipEventSynchronize(t1));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
    last_seconds = ms * 1e-3;
    last_steps = steps;
    sync_all();
}

// ---- load / store / destroy ----

void lbm3d_handle::init_equilibrium() {
    const float c0 = p.density / 3.f, c1 = p.density / 18.f, c2 = p.density / 36.f;
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        s.cur = 0;
        HIP_CHECK(launch_init3d(s.f[0], s.nzs + 2 * GZ3, KS, PL, c0, c1, c2, s.s_comp));
    }
    sync_all();
    loaded = true;
}

void lbm3d_handle::load_cells(const float *aos) {
    if (!aos) throw lbm_failure(LBM_E_INVALID, "cells must not be NULL");
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        const long long n = (long long)s.nzs * p.ny * p.nx;
        const DeviceStage stage(sizeof(float) * Q3 * (size_t)n);
        HIP_CHECK(hipMemcpy(stage.get(), aos + (size_t)s.z0 * p.ny * p.nx * Q3, sizeof(float) * Q3 * (size_t)n,
                            hipMemcpyHostToDevice));
        s.cur = 0;
        HIP_CHECK(launch_aos_to_soa3d(stage.as<float>(), s.o[0], PL, KS, px, p.nx, p.ny, n, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
    }
    refresh();
    loaded = true;
}

void lbm3d_handle::store(float *aos, float *av, int n_av) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "nothing to store");
    sync_all();
    if (aos)
        for (auto &s : slabs) {
            HIP_CHECK(hipSetDevice(s.dev));
            const long long n = (long long)s.nzs * p.ny * p.nx;
            const DeviceStage stage(sizeof(float) * Q3 * (size_t)n);
            HIP_CHECK(launch_soa_to_aos3d(s.o[s.cur], stage.as<float>(), PL, KS, px, p.nx, p.ny, n, s.s_comp));
            HIP_CHECK(hipStreamSynchronize(s.s_comp));
            HIP_CHECK(hipMemcpy(aos + (size_t)s.z0 * p.ny * p.nx * Q3, stage.get(), sizeof(float) * Q3 * (size_t)n,
                                hipMemcpyDeviceToHost));
        }
    if (av && n_av > 0) {
        const int n = std::min(n_av, last_steps);
        std::vector<float> per((size_t)parts * std::max(n, 1), 0.f);
        if (n > 0) {
            if (transport == LBM_TRANSPORT_RCCL) {
                Slab &s = slabs[0];
                HIP_CHECK(hipSetDevice(s.dev));
                const DeviceStage g(sizeof(float) * (size_t)n * world);
                NCCL_CHECK(ncclAllGather(s.av_local, g.get(), (size_t)n, ncclFloat, comm, s.s_comm));
                HIP_CHECK(hipStreamSynchronize(s.s_comm));
                HIP_CHECK(hipMemcpy(per.data(), g.get(), sizeof(float) * (size_t)n * world, hipMemcpyDeviceToHost));
            } else {
                for (auto &s : slabs) {
                    HIP_CHECK(hipSetDevice(s.dev));
                    HIP_CHECK(hipMemcpy(per.data() + (size_t)s.id * n, s.av_local, sizeof(float) * (size_t)n,
                                        hipMemcpyDeviceToHost));
                }
            }
        }
        const float fc = (float)free_cells;
        for (int t = 0; t < n_av; ++t) {
            if (t >= n) {
                av[t] = 0.f;
                continue;
            }
            float tot = 0.f;
            for (int r = 0; r < parts; ++r) tot += per[(size_t)r * n + t];  // fixed slab order
            av[t] = tot / fc;
        }
    }
}

void lbm3d_handle::destroy() {
    walls_release();
    avg_end();
    tracer_end();
    scalar_end();
    forcing_clear();
    sgs_clear();
    grad_release();
    stress_release();
    for (auto &s : slabs) {
        if (hipSetDevice(s.dev) != hipSuccess) continue;
        (void)hipDeviceSynchronize();
        for (int k = 0; k < 2; ++k)
            if (s.f[k] && !(k == 1 && s.f_joint)) (void)hipFree(s.f[k]);
        for (void *q : {(void *)s.obst, (void *)s.obst_g, (void *)s.partials, (void *)s.pass_partials[0],
                        (void *)s.pass_partials[1], (void *)s.av_local})
            if (q) (void)hipFree(q);
        for (hipStream_t st : {s.s_comp, s.s_bnd, s.s_comm})
            if (st) (void)hipStreamDestroy(st);
        for (hipEvent_t e : {s.ev_b, s.ev_i, s.ev_x, s.ev_end})
            if (e) (void)hipEventDestroy(e);
    }
    if (comm) (void)ncclCommDestroy(comm);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
}
