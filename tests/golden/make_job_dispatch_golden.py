"""Records tests/golden/job_dispatch.json: what the device-job dispatcher answered every job of tests/job_dispatch_cases.py —
the refusal's text, or the kernel names, line count and column counts of the job's launch-log lines.  Needs a GPU.

    python tests/golden/make_job_dispatch_golden.py DEBUG_LIBRARY [OUT.json]

DEBUG_LIBRARY is the debug-switch build (-DHIPSOXR_DEBUG_SWITCHES) of the commit the fixture is to pin — the PARENT of a change
to the dispatcher, never the change itself: tests/test_gpu_job_dispatch.py holds the code under test to this file.  The
fixture holds names, counts and texts only — no digests, no timing — so that work on a kernel does not invalidate it; it is
recorded again only when a decision of the dispatcher is changed on purpose.  One child process per environment (the switches
are read once per process)."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
from job_dispatch_cases import CASES, ENVS  # noqa: E402


def main():
    library = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "job_dispatch.json")
    records = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, extra in ENVS.items():
            env = {k: v for k, v in os.environ.items() if not k.startswith("HIPSOXR_")}
            env.update(extra)
            env["HIPSOXR_LIBRARY"] = library
            env["HIPSOXR_DEBUG_LAUNCH_LOG"] = os.path.join(tmp, name + ".log")
            path = os.path.join(tmp, name + ".json")
            subprocess.run([sys.executable, os.path.join(TESTS, "_job_dispatch_probe.py"), name, path], check=True, env=env, timeout=600)
            with open(path) as f:
                records.update(json.load(f))
    assert sorted(records) == sorted(c["name"] for c in CASES), "a case was not run"
    with open(out, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d refused" % (out, len(records), sum("error" in r for r in records.values())))


if __name__ == "__main__":
    main()
