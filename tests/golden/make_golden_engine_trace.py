#!/usr/bin/env python3
"""The golden call trace of pyfft_amd/engine.py: what every entry point hands to the C ABI in both calling modes, over the case table
of tests/engine_trace.py, recorded under its stand-in library (no GPU; the built libspectral.so answers the host-arithmetic entries).

TEST INFRASTRUCTURE.  The trace pins the engine as it stood when this was run, so that a later rewrite of the Python that assembles
the calls can be held to it: the file records the sha256 of that engine.py, and it is not to be regenerated to make a changed engine
pass.  A new case is added by running this against an engine that is known to be right.

Usage:  python tests/golden/make_golden_engine_trace.py        (writes tests/golden/engine_trace.json)
"""
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pytest

import engine_trace
from pyfft_amd import engine


def main():
    mp = pytest.MonkeyPatch()
    try:
        cases = engine_trace.run_table(mp)
    finally:
        mp.undo()
    sha = hashlib.sha256(open(engine.__file__, "rb").read()).hexdigest()
    path = os.path.join(HERE, "engine_trace.json")
    with open(path, "w") as f:                      # one case a line: compact, and a diff names the case
        f.write('{"engine_sha256": "%s",\n "cases": {\n' % sha)
        f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"), sort_keys=True)) for k, v in cases.items()))
        f.write("\n }}\n")
    print("wrote %s: %d cases, %d bytes, engine.py %s" % (path, len(cases), os.path.getsize(path), sha[:16]))


if __name__ == "__main__":
    main()
