"""The fused step's host schedule, observed without a GPU (tools/launch_trace.py): TrainStep built on
the CPU with the library calls, torch.cuda's graphs / streams / events and the collectives replaced
by recorders (every substitution through monkeypatch).  What is checked is what breaks silently on
a GPU: a wait on an event nobody recorded, a gated march without its gate, a fold that does not
wait for its neighbour, eager and captured launches drifting apart."""
import ast
import copy
import importlib.util
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
launch_trace = importlib.util.module_from_spec(spec)
spec.loader.exec_module(launch_trace)

SUBSET = ("default", "parts2", "shard_2rank", "refine_poses", "host_noise_random_bg")


@pytest.fixture(scope="module")
def traces():
    """{configuration: events}, traced once and left unchanged by the tests."""
    mp = pytest.MonkeyPatch()
    try:
        return launch_trace.trace(SUBSET, setattr_=mp.setattr)
    finally:
        mp.undo()


def flat(events):
    """Host order with a capture's events in place (for searches that do not care where a call is)."""
    for e in events:
        yield e
        yield from flat(e.get("events", ()))


def captures(events):
    return {e["graph"]: e["events"] for e in events if e["op"] == "capture"}


def phase(events, name):
    """The events between phase marker `name` and the next one."""
    names = [e.get("name") if e["op"] == "phase" else None for e in events]
    a = names.index(name)
    b = next((i for i in range(a + 1, len(events)) if events[i]["op"] == "phase"), len(events))
    return events[a + 1:b]


def calls(events):
    return [(e["name"], e["args"]) for e in events if e["op"] == "call"]


# ---------------------------------------------------------------------------- the recorder
def test_pointer_into_a_buffer_resolves_to_buffer_and_offset(monkeypatch):
    import torch
    rec = launch_trace.Recorder()
    rec.install(monkeypatch.setattr)
    from mfnerf import engine

    class Root:
        graphs = None
    rec.step = Root()
    a, b = torch.zeros(64), torch.zeros(16, dtype=torch.float16)
    Root.bufs = [a, b]
    engine.call("probe", engine.ptr(a), engine.ptr(a[5:]), engine.ptr(b[3:]), None, engine.ptr(None), 7, 0.5,
                __import__("ctypes").c_void_p(a.data_ptr() + 12), engine.stream())
    (ev,) = rec.document()
    assert ev["name"] == "probe"
    assert ev["args"] == [[0, 0], [0, 20], [1, 6], None, None, 7, 0.5, [0, 12], {"stream": 0}]


def test_two_traces_are_equal_and_a_swap_is_reported(traces, monkeypatch):
    again = launch_trace.trace(("default",), setattr_=monkeypatch.setattr)
    assert launch_trace.dumps(again["default"]) == launch_trace.dumps(traces["default"])
    assert launch_trace.diff(traces["default"], again["default"]) == []
    swapped = copy.deepcopy(traces["default"])
    ev = next(e for e in flat(swapped) if e["op"] == "call" and e["name"] == "mfnerf_field_fw")
    sigma, rgb = ev["args"][8], ev["args"][9]
    assert sigma != rgb
    ev["args"][8], ev["args"][9] = rgb, sigma
    lines = launch_trace.diff(traces["default"], swapped)
    assert len(lines) == 2 and all("mfnerf_field_fw" in ln and "args[" in ln for ln in lines)


# ---------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("name", SUBSET)
def test_every_wait_follows_a_record_of_its_event(traces, name):
    """A wait on a fresh event waits for nothing -- and says nothing."""
    recorded, n_waits = set(), 0
    for e in flat(traces[name]):
        if e["op"] == "record":
            recorded.add(e["event"])
        elif e["op"] == "wait":
            n_waits += 1
            assert e["event"] in recorded, f"{name}: stream {e['stream']} waits on unrecorded event {e['event']}"
    assert n_waits > 0


@pytest.mark.parametrize("name", ("default", "shard_2rank", "refine_poses", "host_noise_random_bg"))
def test_gated_forms_open_the_gate_once_and_the_march_waits_for_it(traces, name):
    ev = traces[name]
    caps = captures(ev)
    (gate,) = {tuple(c[1][0]) for g in ("march_gated[0]", "march_gated[1]") for c in calls(caps[g])[:1]}
    for j in range(2):
        assert calls(caps[f"march_gated[{j}]"])[0][0] == "mfnerf_gate_wait"
    step = "dp_pre" if name == "shard_2rank" else "step"
    for j in range(2):
        opened = 0
        for fn, args in calls(caps[f"{step}[{j}]"]):
            if fn == "mfnerf_gate_signal":
                opened += 1
            elif "grid_encode_bw" in fn:
                opened += sum(1 for a in args if a == list(gate))
        assert opened == 1, f"{name}: {step}[{j}] opens the gate {opened} times"
    # host order: set j's step graph on the main stream, then set 1-j's gated march on the side stream
    replays = [e for e in ev if e["op"] == "replay"]
    seen = 0
    for i, e in enumerate(replays):
        if e["graph"].startswith("march_gated["):
            j = 1 - int(e["graph"][-2])
            before = replays[i - 1]
            assert before["graph"] == f"{step}[{j}]" and before["stream"] != e["stream"]
            assert e["stream"] == next(r["stream"] for r in replays if r["graph"].startswith("march["))
            seen += 1
    assert seen >= 2


def test_each_part_finishes_after_a_wait_on_the_part_before(traces):
    """The folds read-modify-write one gradient: finish[q] only after part q-1's event."""
    ev = traces["parts2"]
    for ph in ("replay0", "replay1", "replay2", "replay3"):
        evs = phase(ev, ph)
        i_fin = {e["graph"]: i for i, e in enumerate(evs) if e["op"] == "replay" and e["graph"].startswith("finish[")}
        assert set(i_fin) == {"finish[0]", "finish[1]"}
        f0, f1 = i_fin["finish[0]"], i_fin["finish[1]"]
        done0 = next(e for e in evs[f0 + 1:] if e["op"] == "record" and e["stream"] == evs[f0]["stream"])
        waits = [i for i, e in enumerate(evs[:f1]) if e["op"] == "wait" and e["stream"] == evs[f1]["stream"]
                 and e["event"] == done0["event"]]
        assert waits, f"{ph}: finish[1] is not ordered after finish[0]"
        assert evs.index(done0) < waits[-1] < f1


def test_eager_launches_equal_the_per_stage_graphs(traces):
    """run() = march[0] + per part (chain, grid_bw, finish) + reduce + update: by entry point,
    argument values and buffer offsets.  Buffers that differ by design: the batch (run()'s own
    against the static set) -- the graphs' copies are compared through run()'s numbering."""
    ev = traces["parts2"]
    caps = captures(ev)
    stages = caps["march[0]"]
    for q in range(2):
        stages = stages + caps[f"chain[0][{q}]"] + caps[f"grid_bw[0][{q}]"] + caps[f"finish[{q}]"]
    stages = stages + caps["reduce"] + caps["update"]
    eager = phase(ev, "run1")
    assert [e["op"] for e in eager] == [e["op"] for e in stages]
    rename = {}  # graph buffer -> eager buffer, which must stay one-to-one
    for a, b in zip(eager, stages):
        assert a.get("name") == b.get("name")
        for x, y in zip(a.get("args", []) + [a.get("dst")], b.get("args", []) + [b.get("dst")]):
            if isinstance(x, list) and isinstance(y, list):
                assert x[1] == y[1], (a["name"], x, y)
                assert rename.setdefault(y[0], x[0]) == x[0], (a["name"], x, y)
            else:
                assert x == y or (isinstance(x, dict) and "stream" in x), (a["name"], x, y)
    assert len(set(rename.values())) == len(rename)
    # only the batch is another buffer in the graphs
    assert sum(1 for k, v in rename.items() if k != v) == 1


# ---------------------------------------------------------------------------- the class
def test_every_attribute_is_defined_in_init():
    from mfnerf import engine
    cls = ast.parse(inspect.getsource(engine)).body
    cls = next(n for n in cls if isinstance(n, ast.ClassDef) and n.name == "TrainStep")

    def targets(fn):
        out = set()
        for n in ast.walk(fn):
            ts = n.targets if isinstance(n, ast.Assign) else [n.target] if isinstance(n, (ast.AugAssign, ast.AnnAssign)) \
                else []
            for t in ts:
                for x in ast.walk(t):
                    if isinstance(x, ast.Attribute) and isinstance(x.value, ast.Name) and x.value.id == "self" \
                            and isinstance(x.ctx, ast.Store):
                        out.add(x.attr)
        return out

    methods = {f.name: targets(f) for f in cls.body if isinstance(f, ast.FunctionDef)}
    # exempt: the pose state, sized by attach_dataset for the dataset's images and absent without
    # refine_poses (test_engine_refine_poses_at_lr_zero_is_the_ray_grads_step asserts that it is)
    pose = methods.pop("_pose_buffers")
    assert pose == {"dR", "dT", "pose_m", "pose_v", "pose_grad", "pose_step_dev", "pose_lr_dev", "pose_buf"}
    late = {f"{m}: self.{a}" for m, ts in methods.items() for a in ts - methods["__init__"] - pose}
    assert not late, sorted(late)
    src = inspect.getsource(engine.TrainStep)
    assert "getattr(" not in src
