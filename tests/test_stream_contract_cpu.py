"""The stream contract is written down three times -- the prototypes of include/tsdgpu.h, the table of DESIGN.md ("The stream
contract") and CONTRACT of tests/stream_order.py, from which tests/test_stream_order_gpu.py takes its asynchronous /
host-synchronous expectations.  They must say the same thing."""
import os
import re

import stream_order as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_entry_points_with_a_stream():
    text = open(os.path.join(ROOT, "include", "tsdgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = set()
    for m in re.finditer(r"\b(?:int|int64_t)\s+(tsdgpu_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"void\s*\*\s*stream\b", m.group(2)):
            out.add(m.group(1))
    return out


def design_table():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 8. The stream contract"):]
    rows = {}
    for m in re.finditer(r"^\| `(tsdgpu_\w+)` \| (asynchronous|host-synchronous) \| (.*?) \|$", sec, flags=re.M):
        assert m.group(1) not in rows, f"{m.group(1)} has two rows"
        rows[m.group(1)] = (m.group(2), m.group(3).strip())
    return rows


def test_every_entry_point_with_a_stream_has_a_row():
    names = header_entry_points_with_a_stream()
    assert len(names) >= 40
    assert names == set(design_table()), sorted(names ^ set(design_table()))
    assert names == set(so.CONTRACT), sorted(names ^ set(so.CONTRACT))


def test_the_tests_expectations_are_the_contract_table():
    rows = design_table()
    for name, kind in so.CONTRACT.items():
        assert rows[name][0] == kind, (name, rows[name][0], kind)


def test_every_host_synchronous_row_gives_its_reason():
    for name, (kind, note) in design_table().items():
        if kind == so.SYNC:
            assert len(note) >= 10, f"{name} is listed host-synchronous without a reason"


def test_the_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "tsdgpu.h")).read()
    head = text[: text.index("#ifndef TSDGPU_H")]
    assert "DESIGN.md" in head and "The stream contract" in head
    # the header says which calls wait on the host although their pointers are device pointers: every such row, by name
    for name, kind in so.CONTRACT.items():
        if kind == so.SYNC:
            assert re.search(r"\b%s\b" % name, head), f"{name} is host-synchronous and the header comment does not name it"
    # ... and names no asynchronous row among them, except where it states that row's remaining wait or its reset_on
    allowed = {"tsdgpu_sos_step", "tsdgpu_resampler_step", "tsdgpu_fir_reset_on", "tsdgpu_sos_reset_on", "tsdgpu_spectrum_reset"}
    for name in set(re.findall(r"\btsdgpu_\w+\b", head)) & set(so.CONTRACT):
        assert so.CONTRACT[name] == so.SYNC or name in allowed, name
    # what reset() requires of work in flight
    assert "null stream" in head and "Synchronise those streams first" in head
