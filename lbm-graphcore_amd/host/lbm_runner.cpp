// lbm_runner -- the reference's LbmRunner CLI (main/LbmRunner.cpp:11-147) on
// top of the HIP engine's C ABI instead of a Poplar Engine.
//
//   lbm_runner --params P --obstacles O [-n N] [--device gpu|loopback|cpu] [-d] [--exe ignored]
//              [--runs 5] [--kernel auto|resident|stream|step2|vec4|scalar|pipeline] [--spl S] [--out-dir DIR]
//              [--tolerance] [--device-fields] [--forces] [--mean-every N] [--gradients] [--stress] [--binned BWxBH]
//              [--tracers FILE [--trace-every N] [--trace-scheme euler|heun]]
//              [--forcing FILE [--forcing-stride N]]
//              [--sgs smagorinsky:CS|omega:W [--sgs-stride N]]
//              [--scalar FILE [--scalar-omega W] [--scalar-stride N] [--buoyancy GX,GY] [--scalar-ref R]
//                             [--transport BWxBH] [--scalar-walls FILE2]]
//              [--json FILE]
//
// Flow (same program numbering as the reference):
//   load params/obstacles -> initialise cells on host -> create engine
//   run(0) ≙ lbm_load_cells -> run(1) ≙ lbm_run (accelerate + maxIters steps)
//   run(2) ≙ lbm_store -> write av_vels.dat / final_state.dat
//   print ==done==, compute time, Reynolds number (av_vels[maxIters-1])
//   then `runs` more lbm_run calls timed by device events (≙ readTimer),
//   reported as MLUPS, GB/s and % of the HBM roofline (and, with --json, as
//   one JSON record); --device-fields makes run(2) lbm_store(av_vels only) +
//   lbm_store_fields and writes final_state.dat from those planar fields (the
//   same bytes); -d prints the lattice's total mass and peak |u| after the
//   run (lbm_field_stats), creates the engine with LBM_FLAG_PROFILE and ends
//   with a per-launch-class device-time summary (≙ engine.printProfileSummary,
//   LbmRunner.cpp:115-122).
// --forces writes forces.dat after the run: the momentum-exchange force the
// fluid put on each obstacle body in the last step (lbm_forces_hip.h; bodies
// = 8-connected periodic components), one `body fx fy links` line per body and
// a final `total` line -- through lbm_set_bodies / lbm_body_forces /
// lbm_wall_force on the GPU, through lbmhost::wallForces with --device cpu.
// --mean-every N runs the first run as lbm_run_steps chunks of N steps (the
// remainder last, the accelerate with the first), samples the time averages
// after each chunk (lbm_averages_hip.h) and writes mean_state.dat after the
// run: `x y mean_ux mean_uy mean_pressure c_uxux c_uxuy c_uyuy c_pp obstacle`
// per cell in final_state.dat's row format; av_vels.dat and final_state.dat
// are the plain run's.
// --gradients writes gradient_state.dat after the run: `x y vorticity
// divergence strain q obstacle` per cell in final_state.dat's row format
// (lbm_gradients_hip.h) -- from lbm_store_gradients on the GPU, from
// lbmhost::velocityGradients of the stored cells with --device cpu.
// --stress writes stress_state.dat after the run: `x y sxx sxy syy strain
// near_wall obstacle` per cell, the values in final_state.dat's format
// (lbm_stress_hip.h) -- from lbm_store_stress on the GPU, from
// lbmhost::neqStrain of the stored cells with --device cpu.
// --binned BWxBH writes binned_state.dat after the run: one row per bin of
// BW x BH cells, `bx by fluid` and the nine sums rho jx jy ux uy speed uxux
// uxuy uyuy in %.12E (lbm_binned_hip.h) -- from lbm_store_binned and
// lbm_bin_fluid_cells on the GPU, from lbmhost::binnedSums of the stored cells
// with --device cpu.
// --tracers FILE reads one seed point `x y` per line (cell units), runs the
// first run in chunks of --trace-every steps (default 10; the chunking rule of
// --mean-every) and moves the points after each chunk by dt = the steps of that
// chunk with --trace-scheme (default heun), then writes tracers.dat after the
// run: `id x y blocked` per point, the positions in %.17g (lbm_tracers_hip.h)
// -- through lbm_tracer_begin / _advance / _store on the GPU, through
// lbmhost::tracerAdvance (lbm_tracer_advance_ref over the stored cells'
// velocities) with --device cpu.
// --scalar FILE reads one cell per line, `x y value [1]` (a trailing 1 makes the
// cell a fixed one: a dye inlet, a heated body; unlisted cells hold 0), runs
// the first run coupled with a passive scalar of relaxation rate
// --scalar-omega (default 1.0) -- --scalar-stride N (default 1) flow steps,
// then as many scalar steps over the frozen lattice, repeated -- and writes
// scalar_state.dat after the run: `x y phi` per cell, x fastest, phi in %.9g
// (lbm_scalar_hip.h).  GPU only.
// --transport BWxBH (with --scalar) writes transport_state.dat after the run:
// one line per bin of BW x BH cells, `bx by fluid` and then the six sums phi
// phiphi uxphi uyphi fx fy in %.17g (lbm_transport_hip.h:
// lbm_scalar_store_binned, lbm_bin_fluid_cells).  GPU only.
// --scalar-walls FILE2 (with --scalar) reads one body per line, `body kind
// value` (kind 0 adiabatic, 1 fixed wall value, 2 fixed flux per link and
// step; bodies numbered as for --forces, unlisted bodies adiabatic), gives the
// bodies those wall models for the run and writes wall_flux.dat after it:
// `body kind value q links` per body, value in %.9g, q -- the scalar the body
// handed to the fluid in the last step -- in %.17g (lbm_scalar_walls_hip.h:
// lbm_scalar_set_walls, lbm_scalar_body_flux).  GPU only.
// --buoyancy GX,GY (with --scalar) lets the scalar drive the flow: ahead of
// every chunk of n <= --scalar-stride steps the momentum
// density * n * (GX, GY) * (phi - R) is added to every fluid cell, R from
// --scalar-ref (default 0) (lbm_thermal_hip.h: lbm_scalar_buoyancy).
// --forcing FILE reads uniform forcing zones, one per line,
// `zone x0 y0 w h lam utx uty fx fy` (lines that start with # are skipped), and
// runs the first run through the forced loop: ahead of every chunk of
// n <= --forcing-stride (default 1) steps every zone is applied as the impulse
// of n steps (lbm_forcing_hip.h: lbm_forcing_apply).  It writes forcing.dat
// after the run: `zone ix iy` per zone, the momentum the zone added summed
// over the run, in %.17g.  The timed re-runs are free runs.  GPU only.
// --sgs smagorinsky:CS | omega:W sets a sub-grid model (a Smagorinsky eddy
// viscosity with the constant CS, or the relaxation rate W everywhere) and runs
// the first run through the LES loop: behind every chunk of
// n <= --sgs-stride (default 1) steps the model is applied for n steps
// (lbm_sgs_hip.h: lbm_sgs_apply).  It writes sgs.dat after the run: per
// application `step cells mean max`, the steps done, the cells the model
// changed and the mean and the largest viscosity it added to them, in %.17g.
// The timed re-runs are free runs.  GPU only.
// --device loopback places all N sub-domains on GPU 0 (the emulator analogue
// of --device ipumodel: exercises the multi-GPU halo path on one device).
// --device cpu runs the same fused step on the host's cores (lbm_cpu.hpp:
// OpenMP rows, bitwise equal to the GPU engine's default numerics); the
// GPU-only options (-n, --tolerance, --kernel, --spl, --graph-steps, --device-fields, --mean-every, --scalar, --buoyancy, --transport, --scalar-walls, --forcing, --sgs) do not
// apply there and are refused with a message.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "lbm_averages_hip.h"
#include "lbm_binned_hip.h"
#include "lbm_cpu.hpp"
#include "lbm_forces_hip.h"
#include "lbm_forcing_hip.h"
#include "lbm_gradients_hip.h"
#include "lbm_host.hpp"
#include "lbm_scalar_hip.h"
#include "lbm_scalar_walls_hip.h"
#include "lbm_sgs_hip.h"
#include "lbm_transport_hip.h"
#include "lbm_stress_hip.h"
#include "lbm_tracers_hip.h"

namespace {

void usage(const char *exe) {
    std::cerr << exe << " - Runs the Lattice Boltzmann D2Q9-BGK engine on MI355X GPUs\n"
              << "Usage:\n  " << exe << " [OPTION...]\n\n"
              << "  -d, --debug          Print per-phase detail\n"
              << "      --device arg     gpu, loopback or cpu (default: gpu)\n"
              << "  -n, --num-gpus arg   number of GPUs / sub-domains to use (default: 1)\n"
              << "      --exe arg        accepted for compatibility with the reference (ignored)\n"
              << "      --params arg     filename of parameters file\n"
              << "      --obstacles arg  filename of obstacles file\n"
              << "      --runs arg       timed re-runs after the first (default: 5)\n"
              << "      --kernel arg     auto, resident, stream, step2, vec4, scalar or pipeline (default: auto; vec4/scalar = one\n"
              << "                       step per launch; pipeline = unfused per-stage kernels)\n"
              << "      --spl arg        stream kernel: time steps per launch, 2..6, 2..10 with --tolerance (default:\n"
              << "                       library choice, 6; 10 with --tolerance)\n"
              << "      --tolerance      fp32 tolerance-mode collision (LBM_FLAG_TOLERANCE: one reciprocal of rho per\n"
              << "                       cell; not bit-identical to the reference, within the tolerance lbm_hip.h states)\n"
              << "      --device-fields  final_state.dat from fields computed on the device (lbm_store_fields: u_x, u_y,\n"
              << "                       |u|, pressure; 16 B per cell to the host instead of 36); same bytes in the file\n"
              << "      --forces         also write forces.dat: drag / lift per obstacle body (momentum exchange of the\n"
              << "                       last step) and their total\n"
              << "      --mean-every arg also write mean_state.dat: time means of u_x, u_y, pressure and their central\n"
              << "                       second moments (Reynolds stresses, pressure variance), sampled on the device\n"
              << "                       every arg steps\n"
              << "      --gradients      also write gradient_state.dat: vorticity, divergence, strain-rate magnitude and\n"
              << "                       the Q criterion (Okubo-Weiss) of the final state\n"
              << "      --stress         also write stress_state.dat: the strain-rate tensor and its magnitude from the\n"
              << "                       non-equilibrium moments of the final state, and the near-wall cells\n"
              << "      --binned arg     BWxBH: also write binned_state.dat: per bin of BW x BH cells the fluid cells and\n"
              << "                       the fp64 sums of rho, rho u, u, |u| and the velocity products of the final state\n"
              << "                       (e.g. NXx1: the profile across the channel; 1xNY: the flux through each section)\n"
              << "      --tracers arg    file of seed points, one `x y` per line in cell units: also write tracers.dat,\n"
              << "                       the points moved with the flow (id x y blocked per point)\n"
              << "      --trace-every arg  steps between two moves of the tracers (default: 10)\n"
              << "      --trace-scheme arg euler or heun (default: heun)\n"
              << "      --scalar arg     file of `x y value [1]` lines (1 = fixed cell; unlisted cells hold 0): carry a\n"
              << "                       passive scalar with the first run and also write scalar_state.dat (x y phi)\n"
              << "      --scalar-omega arg   relaxation rate of the scalar, inside (0, 2) (default: 1.0; the\n"
              << "                       diffusivity is (1/arg - 1/2) / 3)\n"
              << "      --scalar-stride arg  flow steps between two updates of the scalar, which then advances as many\n"
              << "                       steps over the frozen flow (default: 1, the exact coupling)\n"
              << "      --buoyancy arg   GX,GY: with --scalar, the scalar drives the flow -- ahead of every chunk of n steps\n"
              << "                       each fluid cell gains the momentum density * n * (GX, GY) * (phi - ref)\n"
              << "      --scalar-ref arg the ref of --buoyancy (default: 0)\n"
              << "      --scalar-walls arg   file of `body kind value` lines: with --scalar, wall models of the scalar per\n"
              << "                       obstacle body (kind 0 adiabatic, 1 wall value, 2 flux per link and step; bodies as\n"
              << "                       for --forces), and also write wall_flux.dat: body kind value q links\n"
              << "      --transport arg  BWxBH: with --scalar, also write transport_state.dat: per bin of BW x BH cells the\n"
              << "                       fluid cells and the sums of phi, phi^2, ux phi, uy phi and the face fluxes FX, FY\n"
              << "      --forcing arg    file of `zone x0 y0 w h lam utx uty fx fy` lines: forcing zones (a drag lam towards\n"
              << "                       the velocity (utx, uty) and an acceleration (fx, fy) on a box of cells) applied\n"
              << "                       through the first run, and also write forcing.dat: zone ix iy, the momentum added\n"
              << "      --forcing-stride arg  flow steps between two applications of the zones, each the impulse of as\n"
              << "                       many steps (default: 1)\n"
              << "      --sgs arg        smagorinsky:CS or omega:W: a sub-grid model (Smagorinsky constant CS, or the relaxation\n"
              << "                       rate W on every cell) applied through the first run, and also write sgs.dat: step\n"
              << "                       cells mean max, the cells changed and the viscosity added at every application\n"
              << "      --sgs-stride arg flow steps between two applications of the model, each standing for as many steps\n"
              << "                       (default: 1)\n"
              << "      --out-dir arg    directory for av_vels.dat / final_state.dat (default: .)\n"
              << "      --graph-steps arg  replay the step loop as hipGraphs of 2*arg launches (0 = library default, <0 = off)\n"
              << "      --dump-partitioning arg  write the sub-domain decomposition as JSON\n"
              << "      --json arg       append one JSON results record (MLUPS, GB/s, roofline, profile) to this file\n";
}

constexpr double HBM_PEAK_GBS = 8000.0;  // MI355X HBM3E (MI355X_MICROARCH.md)
constexpr double BYTES_PER_UPDATE = 72.0;  // 9 fp32 loads + 9 fp32 stores per cell

std::string json_str(const std::string &v) {
    std::string o = "\"";
    for (char c : v) {
        if (c == '"' || c == '\\') o += '\\';
        if ((unsigned char)c < 0x20) continue;
        o += c;
    }
    return o + "\"";
}

// --device cpu: the reference's program sequence on the host backend
int run_cpu(const lbmhost::Params &params, const lbmhost::Obstacles &obstacles, const std::string &outDir, int runs,
            bool forces, bool gradients, bool stress, int binW, int binH, lbmhost::Tracers *tracers, int traceEvery,
            int traceScheme) {
    std::cout << "Running on the host CPU (" << lbmcpu::Engine::threads()
              << " threads; bitwise numerics: the reference's LastChance.cpp arithmetic)" << std::endl;
    auto cells = lbmhost::initialiseCells(params);
    std::vector<float> av_vels;
    std::unique_ptr<lbmcpu::Engine> e;
    lbmhost::timedStep("Creating engine and loading obstacles", [&]() {
        e = std::make_unique<lbmcpu::Engine>((int)params.nx, (int)params.ny, params.density, params.accel,
                                             params.omega, obstacles.data);
    });
    lbmhost::timedStep("Running copy to device step", [&]() { e->load(cells); });
    double total_compute_time = lbmhost::timedStep("Running LBM", [&]() {
        if (!tracers) {
            e->run((int)params.maxIters, av_vels);
            return;
        }
        // in chunks, the acceleration with the first; the points move after each chunk
        std::vector<float> av;
        for (int done = 0; done < (int)params.maxIters;) {
            const int n = std::min(traceEvery, (int)params.maxIters - done);
            e->run(n, av, done == 0);
            av_vels.insert(av_vels.end(), av.begin(), av.end());
            done += n;
            e->store(cells);
            if (!lbmhost::tracerAdvance(params, obstacles, cells, *tracers, (double)n, traceScheme)) {
                std::cerr << "--tracers: lbm_tracer_advance_ref refused the points" << std::endl;
                std::exit(EXIT_FAILURE);
            }
        }
    });
    lbmhost::timedStep("Running copy to host step", [&]() { e->store(cells); });
    lbmhost::timedStep("Writing output files ", [&]() {
        lbmhost::writeAverageVelocities(outDir + "/av_vels.dat", av_vels);
        lbmhost::writeResults(outDir + "/final_state.dat", params, obstacles, cells);
        if (forces) {
            std::vector<int32_t> labels;
            const int32_t nbodies = lbmhost::labelBodies(obstacles, labels);
            lbmhost::writeForces(outDir + "/forces.dat", lbmhost::wallForces(params, obstacles, cells, labels, nbodies));
        }
        if (gradients) {
            std::vector<float> grads[LBM_GRAD_FIELDS];
            lbmhost::velocityGradients(params, obstacles, cells, grads);
            lbmhost::writeGradientState(outDir + "/gradient_state.dat", params, obstacles, grads);
        }
        if (stress) {
            std::vector<float> strain[LBM_STRESS_FIELDS];
            if (!lbmhost::neqStrain(params, obstacles, cells, strain)) {
                std::cerr << "--stress: omega = 1 leaves no non-equilibrium part in the stored lattice" << std::endl;
                std::exit(EXIT_FAILURE);
            }
            lbmhost::writeStressState(outDir + "/stress_state.dat", params, obstacles, strain,
                                      lbmhost::nearWall(obstacles));
        }
        if (binW > 0)
            lbmhost::writeBinnedState(outDir + "/binned_state.dat",
                                      lbmhost::binnedSums(params, obstacles, cells, (size_t)binW, (size_t)binH));
        if (tracers) {
            lbmhost::tracerBlocked(obstacles, *tracers);
            lbmhost::writeTracers(outDir + "/tracers.dat", *tracers);
        }
    });
    std::cout << "==done==" << std::endl;
    std::cout << "Total compute time was \t" << std::right << std::setw(12) << std::setprecision(5)
              << total_compute_time << "s" << std::endl;
    const float lastAv = params.maxIters > 0 ? av_vels[params.maxIters - 1] : 0.f;
    std::cout << "Reynolds number:  \t" << std::right << std::setw(12) << std::setprecision(12) << std::scientific
              << lbmhost::reynoldsNumber(params, lastAv) << std::endl;
    if (runs > 0) {
        std::cout << "Now doing " << runs << " runs and averaging CPU timing:" << std::endl;
        double secs = 0.0;
        for (int r = 0; r < runs; ++r) {
            e->load(cells);
            secs += e->run((int)params.maxIters, av_vels);
        }
        const double avg = secs / runs;
        std::cout << "Average CPU timing for program is: " << std::fixed << std::setprecision(5) << std::setw(12)
                  << avg << "s" << std::endl;
        std::cout << "MLUPS: " << std::fixed << std::setprecision(1)
                  << (double)params.nx * params.ny * params.maxIters / avg / 1e6 << std::endl;
    }
    return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char *argv[]) {
    std::string paramsFile, obstaclesFile, device = "gpu", exeFile, kernel = "auto", outDir = ".", dumpFile, jsonFile;
    std::string tracersFile, traceSchemeName = "heun";
    int traceEvery = 10;
    std::string scalarFile, wallsFile;
    float scalarOmega = 1.0f;
    int scalarStride = 1;
    bool buoyant = false, scalarRefGiven = false;
    double buoyancyX = 0.0, buoyancyY = 0.0;
    float scalarRef = 0.f;
    int transW = 0, transH = 0;
    std::string forcingFile;
    int forcingStride = 1;
    std::string sgsSpec;
    int sgsMode = LBM_SGS_OFF, sgsStride = 1;
    float sgsCoef = 0.f;
    std::vector<std::string> gpuOnly;  // GPU-only options given on the command line
    int spl = 0;
    int numGpus = 1, runs = 5, graphSteps = 0, meanEvery = 0, binW = 0, binH = 0;
    bool debug = false, tolerance = false, deviceFields = false, forces = false, gradients = false, stress = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        std::string val;
        const auto eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) {
            val = a.substr(eq + 1);
            a = a.substr(0, eq);
        }
        auto next = [&](std::string &dst) -> bool {
            if (!val.empty()) { dst = val; return true; }
            if (i + 1 >= argc) return false;
            dst = argv[++i];
            return true;
        };
        std::string v;
        if (a == "-d" || a == "--debug") {
            debug = true;
        } else if (a == "--device") {
            if (!next(device)) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "-n" || a == "--num-gpus" || a == "--num-ipus") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            numGpus = std::atoi(v.c_str());
            if (numGpus != 1) gpuOnly.push_back(a);
        } else if (a == "--exe") {
            if (!next(exeFile)) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "--params") {
            if (!next(paramsFile)) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "--obstacles") {
            if (!next(obstaclesFile)) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "--runs") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            runs = std::atoi(v.c_str());
        } else if (a == "--kernel") {
            if (!next(kernel)) { usage(argv[0]); return EXIT_FAILURE; }
            if (kernel != "auto" && kernel != "resident" && kernel != "pipeline" && kernel != "stream" && kernel != "step2" && kernel != "vec4" && kernel != "scalar") {
                usage(argv[0]);
                return EXIT_FAILURE;
            }
            gpuOnly.push_back(a);
        } else if (a == "--spl") {
            std::string v;
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            spl = std::atoi(v.c_str());
            gpuOnly.push_back(a);
        } else if (a == "--tolerance") {
            tolerance = true;
            gpuOnly.push_back(a);
        } else if (a == "--device-fields") {
            deviceFields = true;
            gpuOnly.push_back(a);
        } else if (a == "--forces") {
            forces = true;
        } else if (a == "--gradients") {
            gradients = true;
        } else if (a == "--stress") {
            stress = true;
        } else if (a == "--binned") {
            if (!next(v) || sscanf(v.c_str(), "%dx%d", &binW, &binH) != 2) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "--mean-every") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            meanEvery = std::atoi(v.c_str());
            if (meanEvery < 1) { usage(argv[0]); return EXIT_FAILURE; }
            gpuOnly.push_back(a);
        } else if (a == "--tracers") {
            if (!next(tracersFile)) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "--trace-every") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            traceEvery = std::atoi(v.c_str());
            if (traceEvery < 1) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "--trace-scheme") {
            if (!next(traceSchemeName) || (traceSchemeName != "euler" && traceSchemeName != "heun")) {
                usage(argv[0]);
                return EXIT_FAILURE;
            }
        } else if (a == "--scalar") {
            if (!next(scalarFile)) { usage(argv[0]); return EXIT_FAILURE; }
            gpuOnly.push_back(a);
        } else if (a == "--scalar-omega") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            scalarOmega = std::strtof(v.c_str(), nullptr);
            gpuOnly.push_back(a);
        } else if (a == "--scalar-stride") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            scalarStride = std::atoi(v.c_str());
            if (scalarStride < 1) { usage(argv[0]); return EXIT_FAILURE; }
            gpuOnly.push_back(a);
        } else if (a == "--buoyancy") {
            char tail = 0;
            if (!next(v) || sscanf(v.c_str(), "%lf,%lf%c", &buoyancyX, &buoyancyY, &tail) != 2) {
                usage(argv[0]);
                return EXIT_FAILURE;
            }
            buoyant = true;
            gpuOnly.push_back(a);
        } else if (a == "--transport") {
            if (!next(v) || sscanf(v.c_str(), "%dx%d", &transW, &transH) != 2) { usage(argv[0]); return EXIT_FAILURE; }
            gpuOnly.push_back(a);
        } else if (a == "--scalar-walls") {
            if (!next(wallsFile)) { usage(argv[0]); return EXIT_FAILURE; }
            gpuOnly.push_back(a);
        } else if (a == "--scalar-ref") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            scalarRef = std::strtof(v.c_str(), nullptr);
            scalarRefGiven = true;
            gpuOnly.push_back(a);
        } else if (a == "--forcing") {
            if (!next(forcingFile)) { usage(argv[0]); return EXIT_FAILURE; }
            gpuOnly.push_back(a);
        } else if (a == "--forcing-stride") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            forcingStride = std::atoi(v.c_str());
            if (forcingStride < 1) { usage(argv[0]); return EXIT_FAILURE; }
            gpuOnly.push_back(a);
        } else if (a == "--sgs") {
            if (!next(sgsSpec)) { usage(argv[0]); return EXIT_FAILURE; }
            const size_t colon = sgsSpec.find(':');
            const std::string kind = sgsSpec.substr(0, colon);
            char *end = nullptr;
            if (colon != std::string::npos) sgsCoef = std::strtof(sgsSpec.c_str() + colon + 1, &end);
            sgsMode = kind == "smagorinsky" ? LBM_SGS_SMAGORINSKY : kind == "omega" ? LBM_SGS_OMEGA : LBM_SGS_OFF;
            if (sgsMode == LBM_SGS_OFF || !end || end == sgsSpec.c_str() + colon + 1 || *end) {
                std::cerr << "Malformed --sgs (smagorinsky:CS or omega:W): " << sgsSpec << std::endl;
                return EXIT_FAILURE;
            }
            gpuOnly.push_back(a);
        } else if (a == "--sgs-stride") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            sgsStride = std::atoi(v.c_str());
            if (sgsStride < 1) { usage(argv[0]); return EXIT_FAILURE; }
            gpuOnly.push_back(a);
        } else if (a == "--out-dir") {
            if (!next(outDir)) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "--graph-steps") {
            if (!next(v)) { usage(argv[0]); return EXIT_FAILURE; }
            graphSteps = std::atoi(v.c_str());
            gpuOnly.push_back(a);
        } else if (a == "--dump-partitioning") {
            if (!next(dumpFile)) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "--json") {
            if (!next(jsonFile)) { usage(argv[0]); return EXIT_FAILURE; }
        } else if (a == "-h" || a == "--help") {
            usage(argv[0]);
            return EXIT_SUCCESS;
        } else {
            usage(argv[0]);
            return EXIT_FAILURE;
        }
    }
    if (paramsFile.empty() || obstaclesFile.empty() || numGpus < 1 ||
        (device != "gpu" && device != "loopback" && device != "cpu")) {
        usage(argv[0]);
        return EXIT_FAILURE;
    }
    if (debug) std::cout << "Capturing profile information during this run." << std::endl;

    auto params = lbmhost::Params::fromFile(paramsFile);
    if (!params.has_value()) {
        std::cerr << "Could not parse parameters file. Aborting" << std::endl;
        return EXIT_FAILURE;
    }
    auto obstacles = lbmhost::Obstacles::fromFile(params->nx, params->ny, obstaclesFile);
    if (!obstacles.has_value()) {
        std::cerr << "Could not parse obstacles file" << std::endl;
        return EXIT_FAILURE;
    }
    if (binW != 0 || binH != 0) {
        if (binW < 1 || binH < 1 || (size_t)binW > params->nx || (size_t)binH > params->ny) {
            std::cerr << "--binned: bin sizes must lie in 1..nx and 1..ny" << std::endl;
            return EXIT_FAILURE;
        }
    }
    const int traceScheme = traceSchemeName == "euler" ? LBM_TRACER_EULER : LBM_TRACER_HEUN;
    std::optional<lbmhost::Tracers> tracers;
    if (!tracersFile.empty()) {
        if (meanEvery > 0) {
            std::cerr << "--tracers and --mean-every each take the run in their own chunks: give one of them" << std::endl;
            return EXIT_FAILURE;
        }
        tracers = lbmhost::readTracers(tracersFile, *params);
        if (!tracers.has_value()) return EXIT_FAILURE;
    }
    if ((buoyant || scalarRefGiven) && scalarFile.empty()) {
        std::cerr << "--buoyancy and --scalar-ref act on the scalar of --scalar FILE: give it too" << std::endl;
        return EXIT_FAILURE;
    }
    if (transW != 0 || transH != 0) {
        if (scalarFile.empty()) {
            std::cerr << "--transport sums the scalar of --scalar FILE: give it too" << std::endl;
            return EXIT_FAILURE;
        }
        if (transW < 1 || transH < 1 || (size_t)transW > params->nx || (size_t)transH > params->ny) {
            std::cerr << "--transport: bin sizes must lie in 1..nx and 1..ny" << std::endl;
            return EXIT_FAILURE;
        }
    }
    // --scalar-walls: the bodies of --forces with a kind and a value each
    std::vector<int32_t> wallLabels, wallKind;
    std::vector<float> wallValue;
    if (!wallsFile.empty()) {
        if (scalarFile.empty()) {
            std::cerr << "--scalar-walls sets the walls of the scalar of --scalar FILE: give it too" << std::endl;
            return EXIT_FAILURE;
        }
        const int32_t nbodies = lbmhost::labelBodies(*obstacles, wallLabels);
        wallKind.assign(nbodies, LBM_SCALAR_WALL_ADIABATIC);
        wallValue.assign(nbodies, 0.f);
        std::ifstream f(wallsFile);
        if (!f) {
            std::cerr << "Could not read the scalar walls from " << wallsFile << std::endl;
            return EXIT_FAILURE;
        }
        std::string line;
        while (std::getline(f, line)) {
            if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
            long body = -1;
            int kind = -1;
            float value = 0.f;
            if (sscanf(line.c_str(), "%ld %d %f", &body, &kind, &value) != 3 || body < 0 || body >= nbodies ||
                kind < LBM_SCALAR_WALL_ADIABATIC || kind > LBM_SCALAR_WALL_FLUX || !std::isfinite(value)) {
                std::cerr << "Malformed --scalar-walls line (body kind value; body in 0.." << nbodies - 1
                          << ", kind in 0..2, value finite): " << line << std::endl;
                return EXIT_FAILURE;
            }
            wallKind[body] = kind;
            wallValue[body] = value;
        }
    }
    // --scalar: phi0 of every cell and the fixed list
    std::vector<float> scalarPhi, scalarFixedValue;
    std::vector<int32_t> scalarFixedX, scalarFixedY;
    if (!scalarFile.empty()) {
        if (meanEvery > 0 || tracers.has_value()) {
            std::cerr << "--scalar, --tracers and --mean-every each take the run in their own chunks: give one of them"
                      << std::endl;
            return EXIT_FAILURE;
        }
        std::ifstream f(scalarFile);
        if (!f) {
            std::cerr << "Could not read the scalar from " << scalarFile << std::endl;
            return EXIT_FAILURE;
        }
        scalarPhi.assign(params->nx * params->ny, 0.f);
        std::string line;
        while (std::getline(f, line)) {
            if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
            long x = -1, y = -1;
            float value = 0.f;
            int fixed = 0;
            const int got = sscanf(line.c_str(), "%ld %ld %f %d", &x, &y, &value, &fixed);
            if (got < 3 || x < 0 || y < 0 || (size_t)x >= params->nx || (size_t)y >= params->ny ||
                (got == 4 && fixed != 0 && fixed != 1)) {
                std::cerr << "Malformed scalar line (x y value [1] inside the grid expected): " << line << std::endl;
                return EXIT_FAILURE;
            }
            scalarPhi[(size_t)y * params->nx + x] = value;
            if (fixed == 1) {
                scalarFixedX.push_back((int32_t)x);
                scalarFixedY.push_back((int32_t)y);
                scalarFixedValue.push_back(value);
            }
        }
    }
    // --forcing: uniform zones, index and box checked here, the coefficients by the library
    struct ForcingZone {
        int zone, x0, y0, w, h;
        float k[5];
    };
    std::vector<ForcingZone> forcingZones;
    if (!forcingFile.empty()) {
        if (meanEvery > 0 || tracers.has_value() || !scalarFile.empty()) {
            std::cerr << "--forcing, --scalar, --tracers and --mean-every each take the run in their own chunks: give "
                         "one of them" << std::endl;
            return EXIT_FAILURE;
        }
        std::ifstream f(forcingFile);
        if (!f) {
            std::cerr << "--forcing: could not read the zones from " << forcingFile << std::endl;
            return EXIT_FAILURE;
        }
        std::string line;
        while (std::getline(f, line)) {
            const size_t first = line.find_first_not_of(" \t\r");
            if (first == std::string::npos || line[first] == '#') continue;
            ForcingZone z{};
            char tail = 0;
            if (sscanf(line.c_str(), "%d %d %d %d %d %f %f %f %f %f %c", &z.zone, &z.x0, &z.y0, &z.w, &z.h, &z.k[0],
                       &z.k[1], &z.k[2], &z.k[3], &z.k[4], &tail) != 10 ||
                z.zone < 0 || z.zone >= LBM_FORCING_MAX_ZONES) {
                std::cerr << "Malformed --forcing line (zone x0 y0 w h lam utx uty fx fy; zone in 0.."
                          << LBM_FORCING_MAX_ZONES - 1 << "): " << line << std::endl;
                return EXIT_FAILURE;
            }
            if (z.w < 1 || z.h < 1 || z.x0 < 0 || z.y0 < 0 || (size_t)z.x0 + z.w > params->nx ||
                (size_t)z.y0 + z.h > params->ny) {
                std::cerr << "--forcing: the box of zone " << z.zone << " is empty or leaves the domain: " << line
                          << std::endl;
                return EXIT_FAILURE;
            }
            forcingZones.push_back(z);
        }
    }
    if (sgsMode != LBM_SGS_OFF &&
        (meanEvery > 0 || tracers.has_value() || !scalarFile.empty() || !forcingFile.empty())) {
        std::cerr << "--sgs, --forcing, --scalar, --tracers and --mean-every each take the run in their own chunks: give "
                     "one of them" << std::endl;
        return EXIT_FAILURE;
    }
    if (!dumpFile.empty()) {
        // partitioning.json in the layout of grids::serializeToJson
        // (StructuredGridUtils.hpp:135-158), one entry per GPU sub-domain;
        // tile/worker are always 0 here.  Unlike the reference writer the
        // "slice" object is closed, so the file is valid JSON.
        std::vector<lbm_rect> rects(numGpus);
        int32_t R = 0, C = 0;
        if (lbm_partition((int32_t)params->nx, (int32_t)params->ny, numGpus, 0, 0, &R, &C, rects.data()) != LBM_OK) {
            std::cerr << "Cannot partition the grid into " << numGpus << " parts" << std::endl;
            return EXIT_FAILURE;
        }
        std::ofstream f(dumpFile);
        f << R"({"GridPartitioning" : [)" << "\n";
        for (int i = 0; i < numGpus; ++i) {
            if (i) f << ",\n";
            f << "  {\n";
            f << "    \"ipu\":" << i << ",\n";
            f << "    \"tile\":" << 0 << ",\n";
            f << "    \"worker\":" << 0 << ",\n";
            f << "    \"slice\": {\n";
            f << "       \"rows\" : { \"from\" : " << rects[i].y0 << ",\"to\" : " << rects[i].y0 + rects[i].h << "},\n";
            f << "       \"cols\" : { \"from\" : " << rects[i].x0 << ",\"to\" : " << rects[i].x0 + rects[i].w << "}\n";
            f << "    }\n  }";
        }
        f << "\n]}\n";
        std::cout << "Wrote " << R << "x" << C << " decomposition to " << dumpFile << std::endl;
    }
    if (device == "cpu") {
        if (!gpuOnly.empty()) {
            // the host backend has one numerics (bitwise) and one kernel: a
            // '--device cpu --tolerance' run must not silently write bitwise results
            std::cerr << "--device cpu does not take the GPU-only option(s):";
            for (auto &o : gpuOnly) std::cerr << " " << o;
            std::cerr << " (the host backend runs the reference arithmetic on one domain)" << std::endl;
            return EXIT_FAILURE;
        }
        return run_cpu(*params, *obstacles, outDir, runs, forces, gradients, stress, binW, binH,
                       tracers.has_value() ? &*tracers : nullptr, traceEvery, traceScheme);
    }
    const int ndev = lbm_device_count();
    if (ndev <= 0) {
        std::cerr << "No HIP device visible" << std::endl;
        return EXIT_FAILURE;
    }
    if (device == "gpu")
        std::cout << "Running on " << numGpus << " GPU(s)" << std::endl;
    else
        std::cout << "Running " << numGpus << " sub-domain(s) in loop-back on GPU 0" << std::endl;

    double total_compute_time = 0.0;
    auto cells = lbmhost::initialiseCells(*params);
    std::vector<float> av_vels(params->maxIters, 0.0f);

    lbm_handle *h = nullptr;
    const lbm_params abi = params->abi();
    std::vector<int32_t> devs;
    if (device == "loopback") devs.push_back(0);
    lbmhost::timedStep("Creating engine and loading obstacles", [&]() {
        lbm_config cfg{};
        cfg.parts = numGpus;
        cfg.transport = LBM_TRANSPORT_LOCAL;
        cfg.devices = devs.empty() ? nullptr : devs.data();
        cfg.num_devices = (int32_t)devs.size();
        cfg.kernel = kernel == "scalar" ? LBM_KERNEL_SCALAR
                   : kernel == "vec4"   ? LBM_KERNEL_VEC4
                   : kernel == "step2"  ? LBM_KERNEL_STEP2
                   : kernel == "stream" ? LBM_KERNEL_STREAM
                   : kernel == "resident" ? LBM_KERNEL_RESIDENT
                   : kernel == "pipeline" ? LBM_KERNEL_PIPELINE
                                        : LBM_KERNEL_AUTO;
        if (kernel == "scalar" || kernel == "vec4") cfg.flags |= LBM_FLAG_ONE_STEP;
        if (tolerance) cfg.flags |= LBM_FLAG_TOLERANCE;
        if (debug) cfg.flags |= LBM_FLAG_PROFILE;
        cfg.steps_per_launch = spl;
        cfg.graph_steps = graphSteps;
        lbmhost::check(lbm_create_ex(&abi, obstacles->data.data(), &cfg, &h), nullptr, "lbm_create_ex");
    });
    if (debug) {
        std::vector<lbm_rect> rects(numGpus);
        int32_t n = 0;
        lbm_local_rects(h, rects.data(), numGpus, &n);
        for (int i = 0; i < n; ++i)
            std::cout << "sub-domain " << i << ": " << rects[i].w << "x" << rects[i].h << " at (row:" << rects[i].y0
                      << ",col:" << rects[i].x0 << ")" << std::endl;
        const int32_t k = lbm_kernel_in_use(h);
        std::cout << "step kernel: "
                  << (k == LBM_KERNEL_RESIDENT ? "resident" : k == LBM_KERNEL_PIPELINE ? "pipeline" : k == LBM_KERNEL_STREAM ? "stream" : k == LBM_KERNEL_STEP2 ? "step2" : k == LBM_KERNEL_VEC4 ? "vec4" : "scalar")
                  << " (" << lbm_steps_per_launch(h) << " steps per launch)" << std::endl;
    }
    lbmhost::timedStep("Running copy to device step", [&]() {
        lbmhost::check(lbm_load_cells(h, cells.data()), h, "lbm_load_cells");
    });
    double forcingImpulse[LBM_FORCING_MAX_ZONES][2] = {};  // --forcing: forcing.dat's columns
    uint32_t forcingMask = 0;
    struct SgsRow {
        int step;
        double stats[3];
    };
    std::vector<SgsRow> sgsRows;  // --sgs: sgs.dat's lines
    if (meanEvery > 0) {
        total_compute_time += lbmhost::timedStep("Running LBM", [&]() {
            lbmhost::check(lbm_avg_begin(h, LBM_AVG_MEAN | LBM_AVG_SECOND), h, "lbm_avg_begin");
            for (int done = 0; done < (int)params->maxIters;) {
                const int n = std::min(meanEvery, (int)params->maxIters - done);
                lbmhost::check(lbm_run_steps(h, n, done == 0), h, "lbm_run_steps");
                lbmhost::check(lbm_store(h, nullptr, av_vels.data() + done, n), h, "lbm_store");
                lbmhost::check(lbm_avg_sample(h), h, "lbm_avg_sample");
                done += n;
            }
        });
    } else if (tracers.has_value()) {
        total_compute_time += lbmhost::timedStep("Running LBM", [&]() {
            lbmhost::check(lbm_tracer_begin(h, (int64_t)tracers->x.size(), tracers->x.data(), tracers->y.data()), h,
                           "lbm_tracer_begin");
            for (int done = 0; done < (int)params->maxIters;) {
                const int n = std::min(traceEvery, (int)params->maxIters - done);
                lbmhost::check(lbm_run_steps(h, n, done == 0), h, "lbm_run_steps");
                lbmhost::check(lbm_store(h, nullptr, av_vels.data() + done, n), h, "lbm_store");
                lbmhost::check(lbm_tracer_advance(h, (double)n, traceScheme), h, "lbm_tracer_advance");
                done += n;
            }
        });
    } else if (!scalarFile.empty()) {
        total_compute_time += lbmhost::timedStep("Running LBM", [&]() {
            lbmhost::check(lbm_scalar_begin(h, scalarOmega, scalarPhi.data()), h, "lbm_scalar_begin");
            lbmhost::check(lbm_scalar_set_fixed(h, (int64_t)scalarFixedX.size(), scalarFixedX.data(),
                                                scalarFixedY.data(), scalarFixedValue.data()),
                           h, "lbm_scalar_set_fixed");
            if (!wallKind.empty())
                lbmhost::check(lbm_scalar_set_walls(h, wallLabels.data(), (int32_t)wallKind.size(), wallKind.data(),
                                                    wallValue.data()),
                               h, "lbm_scalar_set_walls");
            for (int done = 0; done < (int)params->maxIters;) {
                const int n = std::min(scalarStride, (int)params->maxIters - done);
                if (buoyant)  // the impulse of the chunk's n steps at once
                    lbmhost::check(lbm_scalar_buoyancy(h, (float)(n * buoyancyX), (float)(n * buoyancyY), scalarRef), h,
                                   "lbm_scalar_buoyancy");
                lbmhost::check(lbm_run_steps(h, n, done == 0), h, "lbm_run_steps");
                lbmhost::check(lbm_store(h, nullptr, av_vels.data() + done, n), h, "lbm_store");
                lbmhost::check(lbm_scalar_advance(h, n), h, "lbm_scalar_advance");
                done += n;
            }
        });
    } else if (!forcingFile.empty()) {
        total_compute_time += lbmhost::timedStep("Running LBM", [&]() {
            for (const auto &z : forcingZones)
                lbmhost::check(lbm_forcing_set_zone(h, z.zone, z.x0, z.y0, z.w, z.h, nullptr, z.k), h,
                               "lbm_forcing_set_zone");
            for (int done = 0; done < (int)params->maxIters;) {
                const int n = std::min(forcingStride, (int)params->maxIters - done);
                double impulse[LBM_FORCING_MAX_ZONES][2];
                lbmhost::check(lbm_forcing_apply(h, (float)n, &impulse[0][0]), h, "lbm_forcing_apply");
                for (int z = 0; z < LBM_FORCING_MAX_ZONES; ++z) {
                    forcingImpulse[z][0] += impulse[z][0];
                    forcingImpulse[z][1] += impulse[z][1];
                }
                lbmhost::check(lbm_run_steps(h, n, done == 0), h, "lbm_run_steps");
                lbmhost::check(lbm_store(h, nullptr, av_vels.data() + done, n), h, "lbm_store");
                done += n;
            }
            lbmhost::check(lbm_forcing_zones(h, nullptr, &forcingMask), h, "lbm_forcing_zones");
            lbmhost::check(lbm_forcing_clear(h), h, "lbm_forcing_clear");  // the timed re-runs are free runs
        });
    } else if (sgsMode != LBM_SGS_OFF) {
        total_compute_time += lbmhost::timedStep("Running LBM", [&]() {
            lbmhost::check(lbm_sgs_set(h, sgsMode, sgsCoef, nullptr), h, "lbm_sgs_set");
            for (int done = 0; done < (int)params->maxIters;) {
                const int n = std::min(sgsStride, (int)params->maxIters - done);
                lbmhost::check(lbm_run_steps(h, n, done == 0), h, "lbm_run_steps");
                lbmhost::check(lbm_store(h, nullptr, av_vels.data() + done, n), h, "lbm_store");
                done += n;
                SgsRow row{done, {0.0, 0.0, 0.0}};
                lbmhost::check(lbm_sgs_apply(h, (float)n, row.stats), h, "lbm_sgs_apply");
                sgsRows.push_back(row);
            }
            lbmhost::check(lbm_sgs_set(h, LBM_SGS_OFF, 0.f, nullptr), h, "lbm_sgs_set");  // the timed re-runs are free runs
        });
    } else {
        total_compute_time += lbmhost::timedStep("Running LBM", [&]() { lbmhost::check(lbm_run(h), h, "lbm_run"); });
    }
    std::vector<float> means[LBM_AVG_FIELDS];         // --mean-every: mean_state.dat's columns, planar
    // --mean-every, --tracers, --scalar, --forcing and --sgs gathered av_vels per chunk: the last run's would overwrite them
    float *const avOut =
        (meanEvery > 0 || tracers.has_value() || !scalarFile.empty() || !forcingFile.empty() || sgsMode != LBM_SGS_OFF)
            ? nullptr
            : av_vels.data();
    std::vector<float> f_ux, f_uy, f_u, f_pressure;  // --device-fields: final_state.dat's columns, planar
    lbmhost::BodyForces bodyForces;                   // --forces: forces.dat
    std::vector<float> grads[LBM_GRAD_FIELDS];        // --gradients: gradient_state.dat's columns, planar
    std::vector<float> strain[LBM_STRESS_FIELDS];     // --stress: stress_state.dat's columns, planar
    lbmhost::BinnedSums binned;                       // --binned: binned_state.dat
    std::vector<double> transport[LBM_SBIN_FIELDS];   // --transport: transport_state.dat's columns
    std::vector<int64_t> transportFluid;
    std::vector<double> wallFlux(wallKind.size(), 0.0);       // --scalar-walls: wall_flux.dat's columns
    std::vector<int64_t> wallLinks(wallKind.size(), 0);
    lbmhost::timedStep("Running copy to host step", [&]() {
        if (deviceFields) {
            const size_t n = params->nx * params->ny;
            for (auto *f : {&f_ux, &f_uy, &f_u, &f_pressure}) f->assign(n, 0.f);
            if (avOut) lbmhost::check(lbm_store(h, nullptr, avOut, (int32_t)av_vels.size()), h, "lbm_store");
            lbmhost::check(lbm_store_fields(h, f_ux.data(), f_uy.data(), f_u.data(), f_pressure.data()), h,
                           "lbm_store_fields");
        } else {
            lbmhost::check(lbm_store(h, cells.data(), avOut, (int32_t)av_vels.size()), h, "lbm_store");
        }
        int64_t samples = 0;
        if (meanEvery > 0) lbmhost::check(lbm_avg_samples(h, &samples), h, "lbm_avg_samples");
        if (samples > 0) {
            float *out[LBM_AVG_FIELDS];
            for (int f = 0; f < LBM_AVG_FIELDS; ++f) {
                means[f].assign(params->nx * params->ny, 0.f);
                out[f] = means[f].data();
            }
            lbmhost::check(lbm_avg_store(h, out), h, "lbm_avg_store");
            lbmhost::check(lbm_avg_end(h), h, "lbm_avg_end");
        }
        if (gradients) {
            float *out[LBM_GRAD_FIELDS];
            for (int f = 0; f < LBM_GRAD_FIELDS; ++f) {
                grads[f].assign(params->nx * params->ny, 0.f);
                out[f] = grads[f].data();
            }
            lbmhost::check(lbm_store_gradients(h, out), h, "lbm_store_gradients");
        }
        if (stress) {
            float *out[LBM_STRESS_FIELDS];
            for (int f = 0; f < LBM_STRESS_FIELDS; ++f) {
                strain[f].assign((size_t)params->nx * params->ny, 0.f);
                out[f] = strain[f].data();
            }
            lbmhost::check(lbm_store_stress(h, out), h, "lbm_store_stress");
        }
        if (binW > 0) {
            binned.nbx = LBM_BIN_COUNT(params->nx, (size_t)binW);
            binned.nby = LBM_BIN_COUNT(params->ny, (size_t)binH);
            double *out[LBM_BIN_FIELDS];
            for (int f = 0; f < LBM_BIN_FIELDS; ++f) {
                binned.sum[f].assign(binned.nbx * binned.nby, 0.0);
                out[f] = binned.sum[f].data();
            }
            binned.fluid.assign(binned.nbx * binned.nby, 0);
            lbmhost::check(lbm_store_binned(h, binW, binH, out), h, "lbm_store_binned");
            lbmhost::check(lbm_bin_fluid_cells(h, binW, binH, binned.fluid.data()), h, "lbm_bin_fluid_cells");
        }
        if (tracers.has_value()) {
            tracers->blocked.assign(tracers->x.size(), 0);
            lbmhost::check(lbm_tracer_store(h, tracers->x.data(), tracers->y.data(), tracers->blocked.data()), h,
                           "lbm_tracer_store");
            lbmhost::check(lbm_tracer_end(h), h, "lbm_tracer_end");
        }
        if (transW > 0) {
            const size_t bins = LBM_BIN_COUNT(params->nx, (size_t)transW) * LBM_BIN_COUNT(params->ny, (size_t)transH);
            double *out[LBM_SBIN_FIELDS];
            for (int f = 0; f < LBM_SBIN_FIELDS; ++f) {
                transport[f].assign(bins, 0.0);
                out[f] = transport[f].data();
            }
            transportFluid.assign(bins, 0);
            lbmhost::check(lbm_scalar_store_binned(h, transW, transH, out), h, "lbm_scalar_store_binned");
            lbmhost::check(lbm_bin_fluid_cells(h, transW, transH, transportFluid.data()), h, "lbm_bin_fluid_cells");
        }
        if (!wallKind.empty())
            lbmhost::check(lbm_scalar_body_flux(h, wallFlux.data(), wallLinks.data(), (int32_t)wallKind.size()), h,
                           "lbm_scalar_body_flux");
        if (!scalarFile.empty()) {
            lbmhost::check(lbm_scalar_store(h, scalarPhi.data(), nullptr), h, "lbm_scalar_store");
            lbmhost::check(lbm_scalar_end(h), h, "lbm_scalar_end");
        }
        if (forces) {
            std::vector<int32_t> labels;
            const int32_t nbodies = lbmhost::labelBodies(*obstacles, labels);
            bodyForces.fx.assign(nbodies, 0.0);
            bodyForces.fy.assign(nbodies, 0.0);
            bodyForces.links.assign(nbodies, 0);
            if (nbodies > 0) {
                lbmhost::check(lbm_set_bodies(h, labels.data(), nbodies), h, "lbm_set_bodies");
                lbmhost::check(lbm_body_forces(h, bodyForces.fx.data(), bodyForces.fy.data(), bodyForces.links.data(),
                                               nbodies), h, "lbm_body_forces");
            }
            lbmhost::check(lbm_wall_force(h, &bodyForces.total_fx, &bodyForces.total_fy, &bodyForces.total_links), h,
                           "lbm_wall_force");
        }
    });
    lbmhost::timedStep("Writing output files ", [&]() {
        if (forces) lbmhost::writeForces(outDir + "/forces.dat", bodyForces);
        if (gradients) lbmhost::writeGradientState(outDir + "/gradient_state.dat", *params, *obstacles, grads);
        if (stress)
            lbmhost::writeStressState(outDir + "/stress_state.dat", *params, *obstacles, strain,
                                      lbmhost::nearWall(*obstacles));
        if (binW > 0) lbmhost::writeBinnedState(outDir + "/binned_state.dat", binned);
        if (tracers.has_value()) lbmhost::writeTracers(outDir + "/tracers.dat", *tracers);
        if (!scalarFile.empty()) {
            // scalar_state.dat: `x y phi` per cell, x fastest; %.9g reads back to the same float
            FILE *out = fopen((outDir + "/scalar_state.dat").c_str(), "w");
            if (!out) {
                std::cerr << "Could not write scalar_state.dat" << std::endl;
            } else {
                for (size_t y = 0; y < params->ny; ++y)
                    for (size_t x = 0; x < params->nx; ++x)
                        fprintf(out, "%zu %zu %.9g\n", x, y, (double)scalarPhi[y * params->nx + x]);
                fclose(out);
            }
        }
        if (transW > 0) {
            // transport_state.dat: `bx by fluid` and the six sums per bin, bx fastest; %.17g reads back to the same double
            FILE *out = fopen((outDir + "/transport_state.dat").c_str(), "w");
            if (!out) {
                std::cerr << "Could not write transport_state.dat" << std::endl;
            } else {
                const size_t nbx = LBM_BIN_COUNT(params->nx, (size_t)transW);
                for (size_t b = 0; b < transportFluid.size(); ++b) {
                    fprintf(out, "%zu %zu %lld", b % nbx, b / nbx, (long long)transportFluid[b]);
                    for (int f = 0; f < LBM_SBIN_FIELDS; ++f) fprintf(out, " %.17g", transport[f][b]);
                    fprintf(out, "\n");
                }
                fclose(out);
            }
        }
        if (!wallsFile.empty()) {
            // wall_flux.dat: `body kind value q links` per body; %.9g and %.17g read back to the same float and double
            FILE *out = fopen((outDir + "/wall_flux.dat").c_str(), "w");
            if (!out) {
                std::cerr << "Could not write wall_flux.dat" << std::endl;
            } else {
                for (size_t b = 0; b < wallKind.size(); ++b)
                    fprintf(out, "%zu %d %.9g %.17g %lld\n", b, (int)wallKind[b], (double)wallValue[b], wallFlux[b],
                            (long long)wallLinks[b]);
                fclose(out);
            }
        }
        if (!forcingFile.empty()) {
            // forcing.dat: `zone ix iy` per zone set; %.17g reads back to the same double
            FILE *out = fopen((outDir + "/forcing.dat").c_str(), "w");
            if (!out) {
                std::cerr << "Could not write forcing.dat" << std::endl;
            } else {
                for (int z = 0; z < LBM_FORCING_MAX_ZONES; ++z)
                    if (forcingMask >> z & 1u)
                        fprintf(out, "%d %.17g %.17g\n", z, forcingImpulse[z][0], forcingImpulse[z][1]);
                fclose(out);
            }
        }
        if (sgsMode != LBM_SGS_OFF) {
            // sgs.dat: `step cells mean max` per application; %.17g reads back to the same double
            FILE *out = fopen((outDir + "/sgs.dat").c_str(), "w");
            if (!out) {
                std::cerr << "Could not write sgs.dat" << std::endl;
            } else {
                for (const auto &r : sgsRows)
                    fprintf(out, "%d %lld %.17g %.17g\n", r.step, (long long)r.stats[0],
                            r.stats[0] > 0 ? r.stats[1] / r.stats[0] : 0.0, r.stats[2]);
                fclose(out);
            }
        }
        if (!means[0].empty()) lbmhost::writeMeanState(outDir + "/mean_state.dat", *params, *obstacles, means);
        lbmhost::writeAverageVelocities(outDir + "/av_vels.dat", av_vels);
        if (deviceFields)
            lbmhost::writeResultsFromFields(outDir + "/final_state.dat", *params, *obstacles, f_ux, f_uy, f_u,
                                            f_pressure);
        else
            lbmhost::writeResults(outDir + "/final_state.dat", *params, *obstacles, cells);
    });
    if (debug) {
        // the two numbers a run is watched by: total mass (conserved) and peak speed (Mach-number guard)
        double mass = 0.0;
        float maxSpeed = 0.f;
        lbmhost::check(lbm_field_stats(h, &mass, &maxSpeed), h, "lbm_field_stats");
        char line[96];
        snprintf(line, sizeof(line), "mass: %.12e  max |u|: %.9e", mass, (double)maxSpeed);
        std::cout << line << std::endl;
    }

    std::cout << "==done==" << std::endl;
    std::cout << "Total compute time was \t" << std::right << std::setw(12) << std::setprecision(5)
              << total_compute_time << "s" << std::endl;
    const float lastAv = params->maxIters > 0 ? av_vels[params->maxIters - 1] : 0.f;
    std::cout << "Reynolds number:  \t" << std::right << std::setw(12) << std::setprecision(12) << std::scientific
              << lbmhost::reynoldsNumber(*params, lastAv) << std::endl;

    const int32_t kin = lbm_kernel_in_use(h);
    const char *kname = kin == LBM_KERNEL_RESIDENT ? "resident" : kin == LBM_KERNEL_PIPELINE ? "pipeline"
                      : kin == LBM_KERNEL_STREAM ? "stream" : kin == LBM_KERNEL_STEP2 ? "step2"
                      : kin == LBM_KERNEL_VEC4 ? "vec4" : "scalar";
    const double cells_total = (double)params->nx * params->ny;
    double avg = 0.0, mlups = 0.0, eff_gbs = 0.0, pass_gbs = 0.0;
    int32_t fused_l = 0, single_l = 0;
    if (runs > 0) {
        std::cout << "Now doing " << runs << " runs and averaging GPU-reported timing:" << std::endl;
        double secs = 0.0;
        for (int r = 0; r < runs; ++r) {
            lbmhost::check(lbm_run(h), h, "lbm_run");
            double s = 0.0;
            lbm_last_run_seconds(h, &s);
            secs += s;
        }
        avg = secs / runs;
        mlups = cells_total * params->maxIters / avg / 1e6;
        lbm_run_stats(h, &fused_l, &single_l);
        // 72 B per cell update; a launch that advances S steps
        // moves the lattice through HBM once, so the roofline is per pass
        eff_gbs = BYTES_PER_UPDATE * cells_total * params->maxIters / avg / 1e9;
        std::cout << "Average GPU timing for program is: " << std::fixed << std::setprecision(5) << std::setw(12)
                  << avg << "s" << std::endl;
        std::cout << "MLUPS: " << std::fixed << std::setprecision(1) << mlups << std::endl;
        std::cout << "GB/s (72 B per cell update): " << std::fixed << std::setprecision(1) << eff_gbs << std::endl;
        if (kin == LBM_KERNEL_RESIDENT) {
            std::cout << "HBM roofline: n/a (the resident kernel holds the lattice on chip for the whole run; "
                         "bound by the per-step hand-off between tiles)" << std::endl;
        } else {
            const int passes = fused_l + single_l;
            pass_gbs = BYTES_PER_UPDATE * cells_total * passes / avg / 1e9;
            std::cout << "HBM passes per run: " << passes << " (" << fused_l << " fused launches of up to "
                      << lbm_steps_per_launch(h) << " steps, " << single_l << " one-step)" << std::endl;
            std::cout << "HBM GB/s per lattice pass: " << std::fixed << std::setprecision(1) << pass_gbs << " = "
                      << std::setprecision(1) << 100.0 * pass_gbs / HBM_PEAK_GBS << " % of the "
                      << (int)HBM_PEAK_GBS << " GB/s HBM roofline" << std::endl;
        }
    }
    std::vector<lbm_kernel_time> prof;
    if (debug) {
        int32_t n = 0;
        if (lbm_profile_summary(h, nullptr, 0, &n) == LBM_OK && n > 0) {
            prof.resize(n);
            lbm_profile_summary(h, prof.data(), n, &n);
            std::cout << "Profile summary (device time per launch class over the " << (runs + 1)
                      << " runs; events around every launch):" << std::endl;
            std::cout << "  " << std::left << std::setw(52) << "launch class" << std::right << std::setw(10)
                      << "launches" << std::setw(14) << "total ms" << std::setw(12) << "mean ms" << std::setw(12)
                      << "min ms" << std::setw(12) << "max ms" << std::endl;
            for (const auto &k : prof)
                std::cout << "  " << std::left << std::setw(52) << k.name << std::right << std::setw(10) << k.launches
                          << std::fixed << std::setprecision(3) << std::setw(14) << k.total_ms << std::setw(12)
                          << (k.launches ? k.total_ms / k.launches : 0.0) << std::setw(12) << k.min_ms << std::setw(12)
                          << k.max_ms << std::endl;
        }
    }
    if (!jsonFile.empty()) {
        std::ofstream f(jsonFile, std::ios::app);
        f << "{\"tool\": \"lbm_runner\", \"params\": " << json_str(paramsFile) << ", \"grid\": \"" << params->nx << "x"
          << params->ny << "\", \"steps\": " << params->maxIters << ", \"device\": " << json_str(device)
          << ", \"sub_domains\": " << numGpus << ", \"kernel\": \"" << kname
          << "\", \"steps_per_launch\": " << lbm_steps_per_launch(h)
          << ", \"numerics\": \"" << (lbm_numerics(h) ? "tolerance" : "bitwise") << "\", \"runs\": " << runs
          << std::setprecision(9) << ", \"avg_seconds\": " << avg << std::setprecision(6) << ", \"mlups\": " << mlups
          << ", \"gbs_per_update\": " << eff_gbs << ", \"hbm_passes_per_run\": " << fused_l + single_l
          << ", \"gbs_per_pass\": " << pass_gbs << ", \"hbm_roofline_frac\": "
          << (kin == LBM_KERNEL_RESIDENT || runs <= 0 ? std::string("null") : std::to_string(pass_gbs / HBM_PEAK_GBS))
          << ", \"hbm_peak_gbs\": " << HBM_PEAK_GBS
          << ", \"reynolds\": " << std::scientific << std::setprecision(9) << lbmhost::reynoldsNumber(*params, lastAv)
          << std::defaultfloat << ", \"profile\": [";
        for (size_t i = 0; i < prof.size(); ++i)
            f << (i ? ", " : "") << "{\"name\": " << json_str(prof[i].name) << ", \"launches\": " << prof[i].launches
              << std::setprecision(6) << ", \"total_ms\": " << prof[i].total_ms << ", \"min_ms\": " << prof[i].min_ms
              << ", \"max_ms\": " << prof[i].max_ms << "}";
        f << "]}\n";
        std::cout << "Results record appended to " << jsonFile << std::endl;
    }
    lbm_destroy(h);
    return EXIT_SUCCESS;
}
