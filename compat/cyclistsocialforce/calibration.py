"""cyclistsocialforce.calibration -> cyclistsocialforce_amd.calibration (see the package docstring)"""
from cyclistsocialforce_amd.calibration import *  # noqa: F401,F403
from cyclistsocialforce_amd import calibration as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
