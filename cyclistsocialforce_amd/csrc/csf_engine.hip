// csf_engine.hip - host side of the engine (the C ABI of include/csf.h): ONE translation unit, kept in sections under engine/ -
// the order below is the order of definition (internal helpers in an anonymous namespace, then the extern "C" entry points).

#include "engine/types.inc"   // includes, the RCCL entry points, device buffers, the knobs, struct csf_engine
#include "engine/consts.inc"   // errors, parameter checks, the far-field radius, the rounding bands of a tick, what the kernels derive from a parameter set
#include "engine/road_lattice.inc"   // the lattice over a large road network (csf_road.hip): cells, far-field fit
#include "engine/layout.inc"   // allocation, shard bounds, source chunks, the pair kernel by population size
#include "engine/binning.inc"   // holes left by departures, the re-binning, bounding circles around a pair launch
#include "engine/mirror.inc"   // host mirror <-> device: download, compaction, queue slab, parameter table, upload
#include "engine/gather.inc"   // a sharded run's blocks brought together before the population changes
#include "engine/pending.inc"   // population changes collected for the device (patch_kernel), order and row read-backs
#include "engine/comm_prof.inc"   // the tick's all-gather, per-kernel time stamps
#include "engine/abi_lifetime.inc"   // C ABI: version, errors, csf_create / csf_create_v / csf_destroy
#include "engine/abi_population.inc"   // C ABI: road users arriving and leaving, queues, roads, parameter sets, pushed states
#include "engine/tick.inc"   // one tick enqueued: two launches in turn, one launch (mid-size), side by side (large), one wave (a handful); csf_step, csf_sync
#include "engine/abi_forces_readback.inc"   // C ABI: forces on their own, replay, read-backs, the single-function entry points
#include "engine/abi_fieldmap.inc"   // C ABI: the force field at arbitrary probe points (csf_fieldmap.hip)
#include "engine/abi_sharding.inc"  // C ABI: communicators, loopback groups
#include "engine/abi_batch.inc"   // C ABI: batches of independent scenes (one launch per vehicle class for all one-wave members)
#include "engine/measure.inc"   // what the measures of a recording share: checks, asks, grid, one clear, launches, one copy, one wait, unpacking
#include "engine/abi_encounter.inc"   // C ABI: closest approach and time to collision of a recording (csf_encounter.hip)
#include "engine/abi_pet.inc"   // C ABI: path crossings and post-encroachment time of a recording (csf_pet.hip)
#include "engine/abi_passing.inc"   // C ABI: gaps to the leader, overtakings and meetings of a recording (csf_passing.hip)
#include "engine/abi_flow.inc"      // C ABI: crossings of counting lines, occupancy of areas and of a grid (csf_flow.hip)
#include "engine/abi_clearance.inc" // C ABI: distances to, sides of and crossings of the edges of a road (csf_clearance.hip)
#include "engine/abi_body.inc"   // C ABI: gaps and time to contact between the road users' outlines (csf_body.hip; after abi_encounter.inc, whose split it shares)
#include "engine/abi_calib.inc"   // C ABI: calibration - a resident data set, many parameter sets evaluated per launch (csf_calib.hip)
#include "engine/abi_scene.inc"   // C ABI: calibration on closed-loop scenes - workgroup = (parameter set, scene), the error summed in the launch (csf_scene.hip)
#include "engine/abi_measurement.inc"   // C ABI: far-field radius, time stamps, counters
