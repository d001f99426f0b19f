"""The CAPTURE table of tests/test_gpu_replay.py against the header and the loader: every ``FX3D_API`` function that takes a stream
has a row -- the case that replays it, or the kind of reason it cannot be recorded --, ``_lib.SIGNATURES`` has a pointer where the
header has that stream, and the header's "Capture:" note next to the function states the same as the row.  No device."""
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "flux3d_hip.h")
NEAR = 80   # lines between a note and the declaration it speaks of: "next to its entry point" (a group shares one note)
KINDS = ("replayed", "copies to the host", "host code", "collective")


def _header():
    with open(HEADER) as fh:
        return fh.read()


def _stream_entry_points(text):
    """{name: (line of its declaration, positions of its stream parameters, parameter count)} of the functions that take an
    fx3d_stream_t by value (fx3d_stream_create returns one through a pointer: it takes none)."""
    out = {}
    for m in re.finditer(r"FX3D_API\s+\w+\s+(fx3d_\w+)\(([^;]*?)\);", text, re.S):
        params = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
        at = [i for i, p in enumerate(params) if re.match(r"fx3d_stream_t\s+\w+$", p)]
        if at:
            out[m.group(1)] = (text.count("\n", 0, m.start()) + 1, at, len(params))
    return out


def _notes(text):
    """{name: [(kind, line)]} from the comments that hold "Capture:": each ``fx3d_a, fx3d_b: kind``."""
    out = {}
    for c in re.finditer(r"/\*(.*?)\*/", text, re.S):
        if "Capture:" not in c.group(1):
            continue
        head, body = c.group(1).split("Capture:", 1)
        line = text.count("\n", 0, c.start()) + head.count("\n") + 1
        body = re.sub(r"\s*\n\s*\*\s*", " ", body)
        for m in re.finditer(r"((?:fx3d_\w+(?:, )?)+): (%s)\b" % "|".join(KINDS), body):
            for name in m.group(1).split(", "):
                out.setdefault(name, []).append((m.group(2), line))
    return out


def _case_ids(fn):
    """The ids pytest gives the cases of one test function of tests/test_gpu_replay.py (one parametrisation at most, its ids stated
    or the values themselves)."""
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    if not marks:
        return {fn.__name__}
    assert len(marks) == 1, fn.__name__
    values = marks[0].args[1]
    ids = marks[0].kwargs.get("ids") or [str(v) for v in values]
    assert len(ids) == len(values) and all(isinstance(i, str) for i in ids) and (marks[0].kwargs.get("ids") or all(isinstance(v, (str, int)) for v in values))
    return {f"{fn.__name__}[{i}]" for i in ids}


def test_the_case_ids_are_what_pytest_collects():
    import subprocess
    import sys
    import test_gpu_replay as tr
    r = subprocess.run([sys.executable, "-m", "pytest", tr.__file__, "--collect-only", "-q", "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT)
    collected = {line.split("::", 1)[1] for line in r.stdout.splitlines() if "::" in line}
    mine = set().union(*(_case_ids(fn) for n, fn in vars(tr).items() if n.startswith("test_")))
    assert collected and mine == collected, (sorted(mine - collected), sorted(collected - mine))


def test_what_takes_the_place_of_a_trailing_none_is_the_stream(fx):
    """``_abi`` puts the driver's stream in place of a trailing None wherever the loader's last parameter is a pointer.  Every entry
    point the families and the replay file name whose last parameter is a pointer has the stream there by the header -- but
    fx3d_chamfer_fwd_sharded_async, whose last is the `done` event, which its family always gives."""
    import abi_families as fam
    import test_gpu_replay as tr
    entries = _stream_entry_points(_header())
    def quoted(mod):
        with open(mod.__file__) as fh:
            return set(re.findall(r"\"(fx3d_\w+)\"", fh.read()))
    # (the replay file also names, as rows of its table, the entry points it does not call)
    named = quoted(fam) | (quoted(tr) - {n for n, (kind, _) in tr.CAPTURE.items() if kind != "replayed"})
    named = {n for n in named if n in fx._lib.SIGNATURES and fx._lib.SIGNATURES[n] and fx._lib.SIGNATURES[n][-1] is fx._lib.vp}
    assert len(named) >= 80
    for name in sorted(named - {"fx3d_chamfer_fwd_sharded_async"}):
        assert name in entries and entries[name][1][-1] == entries[name][2] - 1, (name, "its last parameter is a pointer and not the stream")


def test_the_parsers_read_groups_every_kind_and_notes_inside_a_longer_comment():
    text = ("/* x.\n * y (Capture: fx3d_a,\n * fx3d_b: replayed).  More.\n */\n"
            "/* Capture: fx3d_c: copies to the host -- why.  fx3d_d, fx3d_e: host code -- why.  fx3d_f: collective. */\n/* fx3d_g: replayed */")
    assert _notes(text) == {"fx3d_a": [("replayed", 2)], "fx3d_b": [("replayed", 2)], "fx3d_c": [("copies to the host", 5)],
                            "fx3d_d": [("host code", 5)], "fx3d_e": [("host code", 5)], "fx3d_f": [("collective", 5)]}
    decl = ("FX3D_API fx3d_status fx3d_a(int32_t N,\n fx3d_stream_t s);\nFX3D_API fx3d_status fx3d_b(fx3d_stream_t *s);\n"
            "FX3D_API fx3d_status fx3d_c(fx3d_stream_t s, fx3d_stream_t comm_stream, fx3d_event_t e);\nFX3D_API const char *fx3d_d(void);")
    assert _stream_entry_points(decl) == {"fx3d_a": (1, [1], 2), "fx3d_c": (4, [0, 1], 3)}


def test_every_entry_point_that_takes_a_stream_has_a_row_and_the_header_states_the_same(fx):
    import test_gpu_replay as tr
    text = _header()
    entries, notes = _stream_entry_points(text), _notes(text)
    assert len(entries) >= 92
    assert set(tr.CAPTURE) == set(entries), (sorted(set(entries) - set(tr.CAPTURE)), sorted(set(tr.CAPTURE) - set(entries)))
    cases = set().union(*(_case_ids(fn) for n, fn in vars(tr).items() if n.startswith("test_")))
    for name, (kind, what) in tr.CAPTURE.items():
        assert kind in KINDS and isinstance(what, str) and what, name
        if kind == "replayed":   # the case that does it, by its full id: the file's fixture then makes that case record the entry
            assert what in cases, (name, what, "is no case of tests/test_gpu_replay.py")
        sig = fx._lib.SIGNATURES[name]
        line, at, count = entries[name]
        assert len(sig) == count and all(sig[i] is fx._lib.vp for i in at), (name, "the loader's signature has no pointer where the header has the stream")
        assert name in notes, f"{name}: no 'Capture:' note in the header"
        assert len(notes[name]) == 1, (name, notes[name])
        stated, note_line = notes[name][0]
        assert stated == kind, (name, "the header says", stated, "the table", kind)
        assert abs(line - note_line) <= NEAR, (name, "declared at line", line, "its note at line", note_line)
    assert set(notes) <= set(entries), sorted(set(notes) - set(entries))
    # what the drivers put in place of a family's trailing None is the stream: every replayed entry point has it last
    for name, (kind, _) in tr.CAPTURE.items():
        if kind == "replayed":
            line, at, count = entries[name]
            assert at == [count - 1], name


def test_the_old_phrase_is_gone_and_no_case_is_skipped_or_expected_to_fail():
    import test_gpu_replay as tr
    assert "graph-capturable" not in _header()
    with open(tr.__file__) as fh:
        text = fh.read()
    for word in ("pytest.skip", "mark.skip", "xfail", "importorskip"):
        assert word not in text, word
    for obj in vars(tr).values():
        assert all(m.name in ("gpu", "parametrize") for m in getattr(obj, "pytestmark", [])), obj


def test_the_driver_leaves_the_two_other_drivers_calls_as_they_are(fx):
    """``Calls.stream`` is None unless the replay driver runs a call: ``_abi`` then hands the arguments on untouched."""
    import abi_families as fam
    seen = []

    class Fake:
        Flux3DHipError = fx.Flux3DHipError

        class _lib:
            SIGNATURES, vp = fx._lib.SIGNATURES, fx._lib.vp

            @staticmethod
            def call(name, *args):
                seen.append((name, args))
    assert fam.Calls.stream is None
    fam._abi(Fake, "fx3d_knn_gather")(1, 2, 3, 4, 5, 6, 7, None)
    fam.Calls.stream = 99
    try:
        fam._abi(Fake, "fx3d_knn_gather")(1, 2, 3, 4, 5, 6, 7, None)
        fam._abi(Fake, "fx3d_knn_gather")(1, 2, 3, 4, 5, 6, 7, 8)
    finally:
        fam.Calls.stream = None
    assert [a[-1] for _, a in seen] == [None, 99, 8]
