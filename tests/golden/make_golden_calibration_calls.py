"""Records tests/golden/calibration_calls.json - the call transcript of cyclistsocialforce_amd/calibration.py, on the CPU:
    python3 tests/golden/make_golden_calibration_calls.py [output directory]
The fixture was recorded with calibration.py as it was BEFORE it was split into layers; the cases and what an entry holds are in
tests/calibration_calls_common.py.  A case that raises where it should not, or does not raise where it should, ends the recording."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import calibration_calls_common as cc  # noqa: E402


def main(outdir):
    got = cc.transcripts()
    with open(os.path.join(outdir, "calibration_calls.json"), "w") as f:
        json.dump(got, f, separators=(",", ":"))
        f.write("\n")
    for name, log in got.items():
        kinds = [e[0] for e in log]
        print(f"{name}: {kinds.count('call')} calls, {kinds.count('value')} values, {kinds.count('raises')} refusals")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
