// csf_tick_terms.h - device code that the one-wave tick (csf_small_body.inc: small_tick_body) and the 256-thread tick of wide scenes
// (csf_wide_body.inc: wide_tick_body) share, ONCE.  Included by csf_small_body.inc - so inside namespace csf, behind csf_agent_dev.h and
// csf_field.h, as that file is.  A function here holds no shuffle, ballot or barrier and touches nothing another lane owns.
//
// Today that is the Bicycle field's entry of a lane.  The exact pair term, a thread's share of the road term and the switch from a class
// number to agent_body<M> were written as functions of this file too and are NOT here: each computed the parent's bits, and each missed
// another bar - speed, speed, resource figures.  They stay written out in both bodies, with a note at the first copy of each
// ("Folded: the tick terms"; profiles/tick_terms_ab.txt, profiles/tick_terms_resource_usage.txt).
#pragma once

// Bicycle field: (e, 1 / sqrt(1 - e^2)) of a source of speed v (vehicle.py:1062-1064), vref the v_max_riding[1] of its own set.  In fp64
// from the fp64 state; write_record (csf_agent_dev.h) keeps the same pair in rec2 for the pair kernels, formed its own way.
__device__ __forceinline__ float2 bicycle_se(const double v, const double vref) {
    const double e = v > 0.0 ? fmin(pow(v / vref, 0.1), 0.7) : 0.0;
    return make_float2((float)e, (float)(1.0 / sqrt(1.0 - e * e)));
}
