#!/usr/bin/env python3
"""Generates ladder_traces.json: for every kind of ladder one process can hold, the library calls ClassicalTempering makes, and
what it returns, over the call list of tests/recording_engine.py::run_case -- recorded from the tempering.py of the commit BEFORE
the driver's loops were folded into one schedule, and the pin of that refactor: the driver must go on making the same calls.

  python tests/golden/make_ladder_traces.py [--tempering path/to/tempering.py] [--out file]

--tempering loads that file in place of pyisingmontecarlo_amd/tempering.py (an older commit's, say, from `git show`); the rest of
the package (_capi for the host exchange code, distributed) is the tree's.  Needs the built library, no GPU.
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import recording_engine as R  # noqa: E402


class SetAttr:
    """(what run_case needs of pytest's monkeypatch; this process ends with the run)"""
    setattr = staticmethod(setattr)


def load_tempering(path):
    if path is None:
        from pyisingmontecarlo_amd import tempering
        return tempering
    spec = importlib.util.spec_from_file_location("pyisingmontecarlo_amd._tempering_under_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tempering", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "ladder_traces.json"))
    args = ap.parse_args()
    os.environ.pop("ISINGMC_PT_HOST", None)
    tempering = load_tempering(args.tempering)
    cases = [json.dumps(kind) + ": " + json.dumps(R.run_case(tempering, kind, SetAttr), separators=(",", ":")) for kind in R.KINDS]
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(cases) + "\n}\n")


if __name__ == "__main__":
    main()
