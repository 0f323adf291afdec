"""Golden event samples of the window selection, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_segments_golden.py [output directory]
Writes ``segments.json`` (default: next to this file).

``bm/dataset.py`` cannot be imported (mne, dora, flashy, pandas), so the statements of ``_DatasetFactory.apply`` from
``if isinstance(self.condition, str)`` to ``samples = sample_rate.to_ind(times[mask])`` (bm/dataset.py:113-157) are taken
from the reference's source by AST at run time and run, unmodified, as the body of a function of ``(self, recording,
blocks, data, sample_rate)``.  The stubs: ``data`` has ``.times`` = ``np.arange(n_samples) / sample_rate``;
``sample_rate`` is the reference's ``Frequency`` (bm/utils.py); ``self`` carries ``condition``, ``_opts`` and the
switches.  With a float ``condition`` ``recording.events()`` is only copied and sorted (a stub that returns itself); event
times are injected as the ``start`` column of what ``recording.events().query(...)`` returns, under the string condition
``"word"``.  This file holds none of the reference's text.

Every case stores its inputs and ``samples`` (``null``: the reference logged "Empty dataset" and returned None).
"""
import ast
import importlib.util
import json
import logging
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))


def _half_way_times(sample_rate: float):
    """Event times whose sample index is half-way between two integers: x.5 / sample_rate."""
    return [(k + 0.5) / sample_rate for k in (20, 21, 22, 23, 40, 41, 57, 64, 90, 91)]


def cases():
    out = []
    for sr in (120.0, 50.0):
        for cond in (3.0, 0.7):
            out.append(dict(name=f"stride_{cond}_sr{int(sr)}", n_samples=int(31.3 * sr), sample_rate=sr, tmin=-0.5,
                            tmax=2.5, condition=cond, blocks=None, ignore_start_in_block=False,
                            ignore_end_in_block=False))
        out.append(dict(name=f"half_way_sr{int(sr)}", n_samples=int(4 * sr), sample_rate=sr, tmin=-0.1, tmax=0.3,
                        condition=_half_way_times(sr), blocks=None, ignore_start_in_block=False,
                        ignore_end_in_block=False))
    two = [(2.0, 9.5), (14.0, 22.25)]
    three = [(0.0, 4.0), (4.0, 11.0), (20.0, 29.9)]
    for label, blocks in (("two", two), ("three", three)):
        for ig_start in (False, True):
            for ig_end in (False, True):
                out.append(dict(name=f"blocks_{label}_s{int(ig_start)}_e{int(ig_end)}", n_samples=3600,
                                sample_rate=120.0, tmin=-0.5, tmax=2.5, condition=0.7, blocks=blocks,
                                ignore_start_in_block=ig_start, ignore_end_in_block=ig_end))
    out.append(dict(name="too_short", n_samples=300, sample_rate=120.0, tmin=-0.5, tmax=2.5, condition=3.0, blocks=None,
                    ignore_start_in_block=False, ignore_end_in_block=False))
    out.append(dict(name="too_short_events", n_samples=40, sample_rate=20.0, tmin=-0.2, tmax=2.0,
                    condition=[0.1, 0.5, 1.0], blocks=None, ignore_start_in_block=False, ignore_end_in_block=False))
    out.append(dict(name="unsorted_duplicated", n_samples=2400, sample_rate=120.0, tmin=-0.5, tmax=2.5,
                    condition=[5.0, 1.0, 5.0, 3.25, 1.002, 12.5, 0.2, 16.9, 17.0, 3.25, 9.0, 5.004], blocks=None,
                    ignore_start_in_block=False, ignore_end_in_block=False))
    out.append(dict(name="unsorted_blocks", n_samples=2400, sample_rate=50.0, tmin=-0.2, tmax=0.4,
                    condition=[30.0, 2.0, 2.21, 2.19, 11.99, 12.0, 7.7, 2.0, 47.5, 47.7], blocks=[(1.8, 12.4), (29.0, 48.0)],
                    ignore_start_in_block=False, ignore_end_in_block=True))
    return out


def reference_selection():
    """The selection statements of ``_DatasetFactory.apply`` as ``select(self, recording, blocks, data, sample_rate)``,
    which returns ``samples`` (or None through the reference's own ``return None``), and the reference's Frequency."""
    from _ref_import import REF
    path = REF / "bm" / "dataset.py"
    tree = ast.parse(path.read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "_DatasetFactory")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "apply")
    first = next(i for i, st in enumerate(fn.body)
                 if isinstance(st, ast.If) and "self.condition" in ast.unparse(st.test) and "str" in ast.unparse(st.test))
    last = next(i for i, st in enumerate(fn.body)
                if isinstance(st, ast.Assign) and isinstance(st.targets[0], ast.Name) and st.targets[0].id == "samples")
    assert (fn.body[first].lineno, fn.body[last].lineno) == (113, 157), (fn.body[first].lineno, fn.body[last].lineno)
    body = fn.body[first:last + 1] + [ast.Return(value=ast.Name(id="samples", ctx=ast.Load()))]
    args = ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in ("self", "recording", "blocks", "data",
                                                                         "sample_rate")],
                         kwonlyargs=[], kw_defaults=[], defaults=[])
    select = ast.FunctionDef(name="select", args=args, body=body, decorator_list=[], returns=None, type_params=[])
    module = ast.fix_missing_locations(ast.Module(body=[select], type_ignores=[]))
    log = logging.getLogger("make_segments_golden")
    log.setLevel(logging.ERROR)
    scope = {"np": np, "logger": log, "split_wav_as_block": None}
    exec(compile(module, str(path), "exec"), scope)
    spec = importlib.util.spec_from_file_location("bm_ref_utils", REF / "bm" / "utils.py")
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)
    return scope["select"], utils.Frequency


class _Events:
    """``recording.events()``: ``.copy().sort_values('start')`` return the stub; ``.query(...)`` the injected times."""

    def __init__(self, times):
        self.times = times

    def copy(self):
        return self

    def sort_values(self, by):
        assert by == "start"
        return self

    def query(self, query):
        assert self.times is not None, "events queried although the condition is a float"
        return types.SimpleNamespace(start=types.SimpleNamespace(values=np.asarray(self.times, dtype=np.float64)))


def build() -> dict:
    select, Frequency = reference_selection()
    out = []
    for case in cases():
        injected = None if isinstance(case["condition"], float) else case["condition"]
        stub = types.SimpleNamespace(condition=case["condition"] if injected is None else "word",
                                     _opts=dict(tmin=case["tmin"], tmax=case["tmax"], decim=1),
                                     ignore_start_in_block=case["ignore_start_in_block"],
                                     ignore_end_in_block=case["ignore_end_in_block"], split_wav_as_block=False)
        events = _Events(injected)
        recording = types.SimpleNamespace(events=lambda events=events: events, subject_uid="stub")
        data = types.SimpleNamespace(times=np.arange(case["n_samples"]) / case["sample_rate"])
        blocks = None if case["blocks"] is None else [tuple(b) for b in case["blocks"]]
        samples = select(stub, recording, blocks, data, Frequency(case["sample_rate"]))
        out.append(dict(case, samples=None if samples is None else [int(s) for s in samples]))
    return dict(source="bm/dataset.py:113-157", cases=out)


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    (dest / "segments.json").write_text(json.dumps(out, indent=1) + "\n")
    kept = sum(len(c["samples"] or []) for c in out["cases"])
    print(f"segments: {len(out['cases'])} cases, {kept} samples -> {dest / 'segments.json'}")


if __name__ == "__main__":
    main(sys.argv[1:])
