// csf_calib.h — what the calibration kernel (csf_calib.hip: replay_eval_kernel) is handed beside the engine's Dev, shared with
// the host side (engine/abi_calib.inc).
#pragma once
#include "csf_dev.h"

namespace csf {

constexpr int CALIB_MAX_FEAT = 6;   // rows of vehicle.traj an objective can name (calibration.py:352-357)

// The data set of csf_calib_load, resident on the device, and the reset image: every per-slot array that integrate<MODEL> or the
// store section of agent_body writes and a later tick reads, as csf_add_agents left it.  (The position ring hx / hy and the fp32
// records are written too, but nobody reads them in a replay: they are not restored.  zrid and dgood depend on the limits of the
// slot's parameter set - vehicle.py:1732-1736 - and are formed from the image's state and the set of THIS evaluation.)
struct CalibDev {
    const double *Fx, *Fy;       // [n_ticks][n_seq] recorded forces, shared by all parameter sets
    const double *obj;           // [n_ticks][n_seq][n_feat]
    const int32_t *len;          // [n_seq] ticks of every sequence (0 .. n_ticks)
    int32_t n_seq, n_ticks, n_feat;
    int32_t feat[CALIB_MAX_FEAT];   // rows of vehicle.traj (0 .. 5), in the objective's column order
    const double *img_s;         // [STATE_ROWS][cap]
    const double *img_lti;       // [5][cap]
    const double *img_ppsi;      // [cap]
    const int32_t *img_ti;       // [cap]
    const uint32_t *img_status;  // [cap]
    double2 *sums;               // [n_sets * n_seq] (sum d^2, sum |d|) of slot a = set * n_seq + seq: mapped host memory
};

// One launch: slots [0, d.hi) each run their whole sequence.  d is the evaluation's view of the engine (engine/abi_calib.inc).
void launch_replay_eval(const Dev &d, int phases, const CalibDev &c, hipStream_t st);

}  // namespace csf
