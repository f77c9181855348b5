"""No GPU: the case table of tests/test_gpu_streams.py names every C entry that takes a stream.

The entries that take a stream are read from include/aggf.h (a prototype whose last parameter is `stream`) and must be
the ones aggforce_amd/_lib.py:PROTOTYPES ends with a pointer for; each is named by a case's `entries` or by an
exemption with its reason.  A new entry point therefore cannot ship without a gated case."""
import os
import re

import pytest

import test_gpu_streams as S
from aggforce_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_entries():
    text = open(os.path.join(ROOT, "include", "aggf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = set()
    for name, params in re.findall(r"\b(aggf_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        last = params.split(",")[-1].strip()
        if re.search(r"\bstream$", last):
            out.add(name)
    return out


def test_the_header_and_the_binding_agree_on_which_entries_take_a_stream():
    with_stream = stream_entries()
    assert len(with_stream) >= 70, sorted(with_stream)
    assert with_stream <= set(_lib.PROTOTYPES), sorted(with_stream - set(_lib.PROTOTYPES))
    for name in with_stream:
        assert _lib.PROTOTYPES[name][1][-1] is _lib._vp, name


def test_every_entry_that_takes_a_stream_has_a_gated_case_or_a_reasoned_exemption():
    named = {e for c in S.CASES for e in c.entries}
    assert named <= set(_lib.PROTOTYPES), sorted(named - set(_lib.PROTOTYPES))
    missing = sorted(stream_entries() - named - set(S.EXEMPT))
    assert not missing, f"entries with a stream argument that no gated case drives: {missing}"
    assert len(S.EXEMPT) <= S.MAX_EXEMPT and all(len(reason) > 20 for reason in S.EXEMPT.values())


def test_the_case_table_is_well_formed():
    names = [c.name for c in S.CASES]
    assert len(names) == len(set(names))
    for c in S.CASES:
        assert c.entries and c.families and callable(c.build), c.name
        assert (c.synchronises is not None) == (c.name in S.SYNCHRONISES), c.name
    for group in S.GROUPS:
        members = [c for c in S.CASES if c.group == group]
        assert all(not c.synchronises for c in members[:-1]), group  # a waiting call drains the gate: last of its group


@pytest.mark.parametrize("need,want", [(0.0001, 0.02 * 1.25), (0.01, 0.125), (0.045, 0.5)])
def test_gate_length_is_ten_times_the_warm_time_with_headroom_and_a_cap(need, want):
    import stream_gate as SG

    required, requested = SG.gate_length(need)
    assert required == max(10.0 * need, SG.GATE_MIN_S) and requested == pytest.approx(want)
    assert requested <= SG.GATE_MAX_S
