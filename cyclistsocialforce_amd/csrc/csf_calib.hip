// csf_calib.hip — calibration on the device: many parameter sets x many recorded sequences in ONE launch, the error summed here.
//
// Replaces the inner loop of DownhillSimplexCalibration.simulate_single (calibration.py:438-470) and the two error functions
// (calc_sse_timesteps :27-50, calc_maesse_samples :53-77) for one call of the optimiser's objective - or for many of them at
// once: a replay couples no two vehicles, so each (parameter set, sequence) is one dependent chain of ticks and one lane:
//
//   slot a = set * n_seq + seq          its row of the class table is `set` (Dev::cls), so agent_body<MODEL, HET = true> picks it
//   before tick 0                       the slot becomes the fresh vehicle the reference creates per sample (:443-448), from the
//                                       image taken when the data set was loaded (csf_calib.h)
//   t = 0 .. len[seq] - 1               (F_x, F_y) of the recorded tick -> the slot's force rows; PH_INTEGRATE (| PH_FIXSPEED,
//                                       :455-458) through agent_body - the very controller and kinematics of agent_kernel;
//                                       then d = state - objective[t][seq][f] over the objective's features, sum d^2 and
//                                       sum |d| in fp64, in tick order, features in column order
//   at the end                          (sum d^2, sum |d|) -> sums[a] in mapped host memory
//
// The Dev is copied into the kernel and `phases` is an argument, as in agent_kernel: read through a pointer, or with a constant
// phase mask, the compiler contracts a few fp64 chains of some rider classes differently.  What changes from tick
// to tick - Dev::tick, Dev::replay_tick - is set in the lane's own copy, as csf_replay_forces sets it in its view per launch.
// With a history buffer (Dev::hist: the optional trajectories) a lane runs all n_ticks: a finished sequence keeps its last state,
// agent_body's `frozen` path, and is sampled like the others.
#include "csf_agent_dev.h"
#include "csf_calib.h"

namespace csf {

template <int MODEL>
__global__ __launch_bounds__(64) void replay_eval_kernel(const Dev d0, const int phases, const CalibDev c) {
    const uint32_t ka_lines = kernarg_touch<(int)sizeof(Dev) + 4>();
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= d0.hi) return;
    Dev d = d0;
    const int64_t cap = d.cap;
    const int seq = (int)(a % c.n_seq);
    {   // Vehicle.__init__ for this sample (vehicle.py:64-204, 1728-1736): see patch_kernel's spawn
#pragma unroll
        for (int r = 0; r < STATE_ROWS; r++) d.s[r * cap + a] = c.img_s[r * cap + a];
#pragma unroll
        for (int k = 0; k < 5; k++) d.lti[k * cap + a] = c.img_lti[k * cap + a];
        d.ppsi[a] = c.img_ppsi[a];
        d.ti[a] = c.img_ti[a];
        d.status[a] = c.img_status[a];
        const csf_params &p = d.ptab[d.cls[a]];
        const double v = c.img_s[3 * cap + a], delta = c.img_s[4 * cap + a];
        d.zrid[a] = v < p.v_max_walk ? 0 : 1;
        d.dgood[a] = (-p.delta_max_walk < delta && p.delta_max_walk > delta) ? 1 : 0;
    }
    const int len = c.len[seq];
    const int T = d.hist != nullptr ? c.n_ticks : len;
    const int nf = c.n_feat;
    double sse = 0.0, sae = 0.0;
    for (int t = 0; t < T; t++) {
        const int64_t at = (int64_t)t * c.n_seq + seq;
        d.F[a] = c.Fx[at];                                    // (read back by agent_body: this lane's own store, program order)
        d.F[cap + a] = c.Fy[at];
        d.tick = t;                                           // (the sample index counts from the start of the replay)
        d.replay_tick = t;
        agent_body<MODEL, true, false>(d, phases, a, nullptr, ka_lines, 0.0, 0.0);
        if (t < len) {
            const double *o = c.obj + at * nf;
            for (int k = 0; k < nf; k++) {
                const int f = c.feat[k];
                // (a row the class does not have stays zero in the reference's traj: vehicle.py:158-160)
                const double sv = f < d.ns ? d.s[(int64_t)f * cap + a] : 0.0;
                const double e = sv - o[k];                   // a plain difference, no angle wrap: calibration.py:49, 76
                sse += e * e;
                sae += fabs(e);
            }
        }
    }
    c.sums[a] = make_double2(sse, sae);
}

void launch_replay_eval(const Dev &d, int phases, const CalibDev &c, hipStream_t st) {
    if (d.hi <= 0) return;
    const dim3 g((unsigned)((d.hi + 63) / 64)), b(64);
    for_vehicle_class(d.p.model, [&](auto m) { hipLaunchKernelGGL((replay_eval_kernel<decltype(m)::value>), g, b, 0, st, d, phases, c); });
}

}  // namespace csf
