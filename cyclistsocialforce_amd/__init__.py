"""MI355X-native stepping engine for the cyclist social-force model.

Drop-in for the per-tick hot path of chris-konrad/cyclistsocialforce: the same `vehicle.*` constructors,
`.step()` and state arrays, `intersection.SocialForceIntersection` and `scenario.Scenario`, executed by
hand-written HIP kernels (gfx950) behind the C ABI of include/csf.h.  No CPU fallback.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # step_together (intersection.py): many junctions stepped together; imported when first asked for
    if name == "step_together":
        from .intersection import step_together

        return step_together
    if name == "advance_together":                       # ... by many ticks, with the trajectories of all of them
        from .intersection import advance_together

        return advance_together
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["step_together", "advance_together"]
