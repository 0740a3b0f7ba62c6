"""Records tests/golden/local_window_bits.json: every case of tests/local_window_cases.py through the Python API of the
checkout this file lies in, on GPU 0 -- per case the sha256 of the input bytes and of the output bytes -- with the commit
and gdsp_version() of that checkout.  tests/test_local_window_bits.py then holds every later build to these bits.

Run it from a built checkout of the commit whose bits are to be kept: the parent of a change that must not move them.

    timeout -k 10 300 python tools/record_local_window_bits.py [--out <file>]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "local_window_bits.json"))
    ap.add_argument("--commit", default=None, help="the commit of this checkout, where it is no git work tree of its own")
    args = ap.parse_args()
    import genodsp_amd as gd
    import local_window_cases as lw
    gd.set_device(0)
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    record = {"commit": commit, "gdsp_version": gd.lib().gdsp_version().decode(), "cases": {}}
    for case in lw.cases():
        record["cases"][case.id] = {"input": lw.input_digest(case), "output": lw.output_digest(gd, case)}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases on %s (%s) -> %s" % (len(record["cases"]), commit[:12], record["gdsp_version"], args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
