"""Do the aimed sources of tests/dfast_sources.py bite? Every entry of tests/dfast_mutants.py -- a one-token change of a decision inside a double-fast search -- is applied to a
COPY of the encoder header in a temporary directory, tests/emu/emu_dfast.cpp is compiled against that copy for the host, and a child process runs the aimed sources against it
under a time limit: the mutant's parse must differ from libzstd's in every form the entry names, on at least one source OF THE FAMILY AIMED AT IT
(dfast_mutants.family_of): aimed means kills it. An entry marked equivalent must survive all of them.

Mutated code is never compiled for, copied to or run on a GPU: this module has no `gpu` mark, builds with g++ only and writes nothing into the repository."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import dfast_mutants as dm
from tests.dfast_check import FORMS, build_emu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "python-zstandard_amd", "csrc")
HEADER = os.path.join(CSRC, "zhip_encode_kernel.hpp")
JOBS = 8
CHILD_LIMIT = 300          # seconds; a full run of the sources takes about 10


def _one(args):
    index, work = args
    name, old, new, verdict = dm.MUTANTS[index]
    text = dm.apply(open(HEADER).read(), old, new)
    if text is None: return "stale"
    d = os.path.join(work, "m%02d" % index)
    os.makedirs(d)
    header = os.path.join(d, "zhip_encode_kernel.hpp")
    open(header, "w").write(text)
    try:
        lib = build_emu(d, header=header)
    except subprocess.CalledProcessError:
        return "does not compile"
    forms = FORMS if isinstance(verdict, str) else verdict
    try:
        r = subprocess.run([sys.executable, "-m", "tests.dfast_mutants", lib, ",".join(forms), (None if isinstance(verdict, str) else dm.family_of(name)) or "all"], cwd=ROOT, capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        return "the child ran into its time limit"
    if r.returncode != 0: return "the child failed: " + r.stderr[-600:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    from tests import reflib
    if not reflib.have_ref():
        pytest.skip("no libzstd 1.5.7 available")
    work = str(tmp_path_factory.mktemp("dfast_mutants"))
    with ThreadPoolExecutor(JOBS) as pool:
        out = list(pool.map(_one, [(i, work) for i in range(len(dm.MUTANTS))]))
    return out


def test_the_list_names_each_decision_once():
    names = [m[0] for m in dm.MUTANTS]
    assert len(set(names)) == len(names) and len(names) >= 30
    text = open(HEADER).read()
    for name, old, new, verdict in dm.MUTANTS:
        assert text.count(old) == 1, "stale: %r is in the header %d times, not once" % (name, text.count(old))
        assert old != new and (isinstance(verdict, str) and verdict.startswith("equivalent: ") and len(verdict) > 60 or set(verdict) <= set(FORMS))


@pytest.mark.parametrize("index", range(len(dm.MUTANTS)), ids=[m[0].replace(" ", "_") for m in dm.MUTANTS])
def test_mutant(results, index):
    name, old, new, verdict = dm.MUTANTS[index]
    got = results[index]
    assert isinstance(got, dict), "%s: %s" % (name, got)
    if isinstance(verdict, str):
        assert not got, "%s is marked equivalent but %r tell it from libzstd, so the reason given is wrong: %s" % (name, got, verdict)
    else:
        survived = [f for f in verdict if f not in got]
        assert not survived, "%s survives every source of the family aimed at it (%s) in %s (killed in %r)" % (name, dm.family_of(name) or "all", survived, got)
