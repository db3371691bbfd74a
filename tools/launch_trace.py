#!/usr/bin/env python3
"""Record the host schedule of the fused training step without a GPU.

    tools/launch_trace.py [-o TRACE.json] [--root CHECKOUT] [--config NAME ...]
    tools/launch_trace.py --diff OLD.json NEW.json

TrainStep is built on the CPU with mfnerf._lib's call / ptr / stream (and the names imported from
it into mfnerf.engine and mfnerf.data), torch.cuda's graphs, streams and events and mfnerf.dp's
collectives replaced by recorders; the library's size queries are real, so libmfnerf_hip.so must be
built.  For a fixed matrix of configurations (CONFIGS) one script (run x2, capture, replay x4,
occupancy refresh x4) is driven and everything the host issued is written in host order:

  call     a library call: entry point, stream, arguments.  Scalars by value, NULL as null, the grid
           descriptor and mfnerf_adam_fused by their fields, every pointer -- raw addresses included
           -- as [buffer, byte offset], a buffer being a tensor storage numbered by its first
           appearance in the configuration's trace (so a renamed attribute does not show; a swapped,
           aliased or re-offset buffer does)
  capture  a graph capture under its key path in TrainStep.graphs ("chain[1][0]", "occ[...]"), the
           events captured into it, whether the generator state was registered
  replay / wait / record / collective
           graph replays, stream waits, event records and collectives with the stream they were
           issued on; streams and events numbered by first appearance
  torch    a torch op that writes one of the step's buffers: op name and destination
  phase    the script's position (run0, capture, replay1, ...)

Two traces of one tree are byte-identical; --diff lists where two traces differ (exit status 1).
--root traces another checkout of this repository with this recorder (a refactor's before/after; it
needs its own built library, or MFNERF_LIB pointing at one with the same ABI)."""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(n_rays=256, max_samples=8, log2_T=16)  # the smallest shapes that still take each branch
# name -> options: cfg (StepConfig fields), dataset, shard (rank, world[, force]), exchange,
# host_noise, rccl (dp.direct_rccl faked), extra_run (a closing run(optimize=False))
CONFIGS = {
    "default": dict(extra_run=True),
    "parts2": dict(cfg=dict(n_parts=2)),
    "parts4": dict(cfg=dict(n_parts=4)),
    "distortion": dict(cfg=dict(lambda_distortion=1e-3)),
    "ray_grads": dict(cfg=dict(ray_grads=True)),
    "mixed128": dict(cfg=dict(grid="MixedFeature", N_tables=8, rgb_width=128)),
    "random_bg_dataset": dict(cfg=dict(random_bg=True, scale=4.0), dataset=True),
    "refine_poses": dict(cfg=dict(refine_poses=True), dataset=True),
    "unbinned": dict(cfg=dict(binned_grid=False)),
    "float_atomics": dict(cfg=dict(fixed_point_grid=False)),
    "no_amp": dict(cfg=dict(skip_nonfinite=False, dynamic_loss_scale=False)),
    "shard_1rank": dict(shard=(0, 1, True)),
    "shard_2rank": dict(shard=(0, 2)),
    "shard_no_amp": dict(cfg=dict(skip_nonfinite=False, dynamic_loss_scale=False), shard=(0, 2)),
    "allreduce": dict(exchange=True),
    "host_noise": dict(host_noise=True),
    "host_noise_random_bg": dict(cfg=dict(random_bg=True, scale=4.0), host_noise=True),
    "rccl_shard": dict(shard=(0, 2), rccl=True),
    "rccl_allreduce": dict(exchange=True, rccl=True),
}


# ---------------------------------------------------------------------------- the recorder
class Stream:
    def __init__(self, rec, **_kw):
        self.rec = rec

    def wait_event(self, ev):
        self.rec.emit(op="wait", stream=self, event=ev)


class Event:
    def __init__(self, rec):
        self.rec = rec

    def record(self, stream=None):
        self.rec.emit(op="record", stream=stream or self.rec.cur, event=self)


class Graph:
    def __init__(self, rec):
        self.rec, self.rng, self.events = rec, False, None

    def register_generator_state(self, _gen):
        self.rng = True

    def replay(self):
        self.rec.emit(op="replay", stream=self.rec.cur, graph=self)


class _StreamArg:
    """What the fake stream() hands to call(): the stream the launch goes to."""

    def __init__(self, stream):
        self.stream = stream


class Recorder:
    """The substitutes and the event log.  install(setattr) puts the substitutes in place through
    the given setter (pytest's monkeypatch.setattr, or Patches.set)."""

    def __init__(self):
        self.events = []
        self.main = Stream(self)
        self.cur = self.main
        self.step = None          # root of the object walk that finds the step's storages
        self.extra_roots = []
        self._bufs = {}           # storage address -> (nbytes, storage): kept alive, so no address is reused
        self.rccl = False

    # -- substitutes
    def install(self, setattr_):
        import torch
        from mfnerf import _lib, data, dp, engine
        for mod in (_lib, engine, data):
            setattr_(mod, "call", self.call)
            setattr_(mod, "ptr", self.ptr)
            setattr_(mod, "stream", self.stream_arg)
        tc = torch.cuda
        setattr_(tc, "CUDAGraph", lambda: Graph(self))
        setattr_(tc, "graph", self.capture)
        setattr_(tc, "graph_pool_handle", lambda: None)
        setattr_(tc, "synchronize", lambda *a: None)
        setattr_(tc, "Stream", lambda **kw: Stream(self, **kw))
        setattr_(tc, "Event", lambda **kw: Event(self))
        setattr_(tc, "current_stream", lambda *a: self.cur)
        setattr_(tc, "stream", self.on_stream)
        for name in ("reduce_scatter_mean_", "all_gather_", "allreduce_mean_"):
            setattr_(dp, name, self._collective(name))
        setattr_(dp, "direct_rccl", lambda: object() if self.rccl else None)

    def emit(self, **ev):
        self.events.append(ev)

    def phase(self, name):
        self.emit(op="phase", name=name)

    def ptr(self, t):
        if t is None:
            return ctypes.c_void_p(0)
        self._add(t)
        return ctypes.c_void_p(t.data_ptr())

    def stream_arg(self):
        return _StreamArg(self.cur)

    def call(self, name, *args):
        self.emit(op="call", name=name, stream=self.cur, args=[self._arg(a) for a in args])

    @contextlib.contextmanager
    def capture(self, g, pool=None):
        n = len(self.events)
        yield
        g.events = self.events[n:]
        del self.events[n:]
        self.emit(op="capture", graph=g)

    @contextlib.contextmanager
    def on_stream(self, s):
        old, self.cur = self.cur, s
        try:
            yield
        finally:
            self.cur = old

    def _collective(self, name):
        def fn(*args):
            import torch
            self.emit(op="collective", name=name, stream=self.cur,
                      args=[self._addr(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args])
            return args[0]
        fn.__name__ = name
        return fn

    # -- pointers
    def _add(self, t):
        s = t.untyped_storage()
        if s.nbytes():
            self._bufs[s.data_ptr()] = (s.nbytes(), s)

    def _walk(self, o, seen):
        import torch
        if id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            self._add(o)
        elif isinstance(o, (list, tuple)):
            for x in o:
                self._walk(x, seen)
        elif isinstance(o, dict):
            for x in o.values():
                self._walk(x, seen)
        elif hasattr(o, "__dict__") and type(o).__module__.startswith("mfnerf"):
            self._walk(vars(o), seen)

    def _find(self, addr):
        for base, (n, _s) in self._bufs.items():
            if base <= addr < base + n:
                return [base, addr - base]
        return None

    def _addr(self, addr, strict=True):
        """[storage address, byte offset] of a raw address (the address becomes the buffer's number
        when the trace is written); a miss rescans the step for storages not seen yet."""
        if not addr:
            return None
        hit = self._find(addr)
        if hit is None:
            seen = set()
            for root in [self.step] + self.extra_roots:
                self._walk(root, seen)
            hit = self._find(addr)
        if hit is None and strict:
            raise LookupError(f"pointer {addr:#x} is in no storage of the step")
        return hit and {"buf": hit[0], "off": hit[1]}

    def _struct(self, s):
        out = {}
        for name, ctype in s._fields_:
            v = getattr(s, name)
            if ctype is ctypes.c_void_p:
                v = self._addr(v)
            elif isinstance(v, ctypes.Array):
                v = list(v)
            out[name] = v
        return {type(s).__name__: out}

    def _arg(self, a):
        if a is None:
            return None
        if isinstance(a, _StreamArg):
            return {"stream": a.stream}
        if isinstance(a, ctypes.c_void_p):
            return self._addr(a.value)
        if isinstance(a, ctypes.Structure):
            return self._struct(a)
        if hasattr(a, "_obj") and isinstance(a._obj, ctypes.Structure):  # ctypes.byref(structure)
            return self._struct(a._obj)
        if isinstance(a, (bool, int, float, str)):
            return a
        raise TypeError(f"unrecorded argument type {type(a).__name__}")

    # -- torch ops that write one of the step's buffers
    @contextlib.contextmanager
    def torch_ops(self):
        from torch.utils._python_dispatch import TorchDispatchMode
        import torch
        rec = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                kwargs = kwargs or {}
                out = func(*args, **kwargs)
                sch = func._schema.arguments
                for i, a in enumerate(sch):
                    if a.alias_info is None or not a.alias_info.is_write:
                        continue
                    v = kwargs.get(a.name, args[i] if i < len(args) else None)
                    if isinstance(v, torch.Tensor) and v.numel():
                        dst = rec._addr(v.data_ptr(), strict=False)
                        if dst is not None:
                            rec.emit(op="torch", name=str(func), stream=rec.cur, dst=dst)
                return out

        with Mode():
            yield

    # -- the document
    def document(self):
        """The events as JSON-ready data: buffers, streams, events numbered by first appearance in
        host order (a captured graph's events at its capture), graphs by their key path."""
        names = {}

        def name_graphs(o, path):
            if isinstance(o, Graph):
                names.setdefault(id(o), path)
            elif isinstance(o, (list, tuple)):
                for i, x in enumerate(o):
                    name_graphs(x, f"{path}[{i}]")
            elif isinstance(o, dict):
                for k, x in o.items():
                    name_graphs(x, f"{path}[{k!r}]" if path else str(k))

        name_graphs(self.step.graphs or {}, "")
        occ = vars(self.step).get("_occ")
        if occ is not None:
            name_graphs(occ.graphs, "occ")
        numbers = {"buf": {}, Stream: {}, Event: {}}

        def number(kind, key):
            return numbers[kind].setdefault(key, len(numbers[kind]))

        def conv(v):
            if isinstance(v, dict):
                if set(v) == {"buf", "off"}:
                    return [number("buf", v["buf"]), v["off"]]
                return {k: conv(x) for k, x in v.items()}
            if isinstance(v, list):
                return [conv(x) for x in v]
            if isinstance(v, (Stream, Event)):
                return number(type(v), id(v))
            if isinstance(v, Graph):
                return names.get(id(v), "?")
            return v

        out = []
        for ev in self.events:
            e = conv(ev)
            if ev["op"] == "capture":
                e["rng"] = ev["graph"].rng
                e["events"] = [conv(x) for x in ev["graph"].events]
            out.append(e)
        return out


class Patches:
    """setattr with an undo list, for use outside pytest."""

    def __init__(self):
        self.undo = []

    def set(self, obj, name, value):
        self.undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def restore(self):
        for obj, name, value in reversed(self.undo):
            setattr(obj, name, value)
        self.undo.clear()


# ---------------------------------------------------------------------------- the script
def trace_config(rec, name):
    """Drive the script of configuration `name` against an installed recorder; returns the trace's
    events (Recorder.document)."""
    import torch
    from mfnerf import dp, engine
    from mfnerf.data import DeviceDataset
    o = CONFIGS[name]
    gen = torch.Generator().manual_seed(0)  # (the values do not matter to the trace)
    rec.rccl = bool(o.get("rccl"))
    cfg = engine.StepConfig(**{**BASE, **o.get("cfg", {})})
    rec.phase("setup")
    st = rec.step = engine.TrainStep(cfg, device="cpu")
    if o.get("shard"):
        st.shard_optimizer(*o["shard"][:2], force=len(o["shard"]) > 2)
    exchange = dp.allreduce_mean_ if o.get("exchange") else None
    host_noise = bool(o.get("host_noise"))
    b = [None] * 3
    if o.get("dataset"):
        n, hw = 3, 8 * 8
        st.attach_dataset(DeviceDataset(torch.rand(n, hw, 3, generator=gen), torch.eye(4)[:3].repeat(n, 1, 1),
                                        torch.rand(hw, 3, generator=gen), device="cpu"))
    else:
        b = st.make_batches(3)
    noise = [torch.rand(cfg.n_rays, generator=gen) for _ in range(3)] if host_noise else [None] * 3
    bg = [(0.25 * i, 0.5, 0.75) for i in range(3)] if host_noise and st._random_bg() else [None] * 3
    grid_bw_events = (Event(rec), [Event(rec) for _ in range(cfg.n_parts)])
    count_grid = torch.zeros(st.cascades, st.G ** 3)
    rec.extra_roots = [b, noise, count_grid]
    with rec.torch_ops():
        for i in range(2):
            rec.phase(f"run{i}")
            st.run(b[0], exchange=exchange)
        rec.phase("capture")
        st.capture(host_noise=host_noise)
        for i in range(4):
            rec.phase(f"replay{i}")
            k, kn = i % 3, (i + 1) % 3
            kw = dict(exchange=exchange, noise=noise[k], bg=bg[k])
            if i == 1:
                kw["grid_bw_events"] = grid_bw_events
            if i == 3:
                kw["prefetch"] = False
            else:
                kw.update(next_batch=b[kn], next_noise=noise[kn], next_bg=bg[kn])
            st.replay(b[k], **kw)
        for i, kw in enumerate((dict(warmup=True), dict(warmup=False), dict(warmup=False),
                                dict(warmup=False, count_grid=count_grid))):
            rec.phase(f"occupancy{i}")
            st.update_density_grid(**kw)
        if o.get("extra_run"):
            rec.phase("run_no_optimize")
            st.run(b[0], optimize=False)
    return rec.document()


def trace(names=None, setattr_=None):
    """{configuration: events} for the named configurations (default: the whole matrix).  setattr_:
    how to put the substitutes in place (default: set here, restored on return)."""
    out = {}
    for name in names or CONFIGS:
        patches = Patches() if setattr_ is None else None
        rec = Recorder()
        rec.install(patches.set if patches else setattr_)
        try:
            out[name] = trace_config(rec, name)
        finally:
            if patches:
                patches.restore()
    return out


def count_events(events):
    return sum(1 + count_events(e.get("events", ())) for e in events)


def dumps(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


# ---------------------------------------------------------------------------- the comparer
def diff(a, b, path=""):
    """Where two traces (or any parts of them) differ: a list of 'path: a | b' lines."""
    if type(a) is not type(b):
        return [f"{path}: {a!r} | {b!r}"]
    if isinstance(a, dict):
        out = []
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                out.append(f"{path}.{k}: only in the {'first' if k in a else 'second'}")
            else:
                out += diff(a[k], b[k], f"{path}.{k}")
        return out
    if isinstance(a, list):
        what = a[0].get("name", a[0].get("graph", "")) if a and isinstance(a[0], dict) else ""
        out = [f"{path}: {len(a)} | {len(b)} entries {what}"] if len(a) != len(b) else []
        for i, (x, y) in enumerate(zip(a, b)):
            tag = x.get("name") or x.get("graph") or x.get("op") if isinstance(x, dict) else None
            out += diff(x, y, f"{path}[{i}{':' + str(tag) if tag else ''}]")
        return out
    return [] if a == b else [f"{path}: {a!r} | {b!r}"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-o", "--out", help="write the JSON document here (default: only the summary)")
    ap.add_argument("--root", default=ROOT, help="the checkout whose mf-nerf_amd/mfnerf is traced")
    ap.add_argument("--config", action="append", choices=list(CONFIGS), help="default: the whole matrix")
    ap.add_argument("--diff", nargs=2, metavar=("OLD", "NEW"))
    args = ap.parse_args(argv)
    if args.diff:
        lines = diff(*(json.load(open(p)) for p in args.diff))
        print("\n".join(lines[:200]) if lines else "identical")
        return 1 if lines else 0
    sys.path[:0] = [args.root, os.path.join(args.root, "mf-nerf_amd")]
    doc = trace(args.config)
    text = dumps(doc)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    for name, events in doc.items():
        print(f"{name:22s} {count_events(events):5d} events")
    print(f"{len(doc)} configurations, {sum(count_events(e) for e in doc.values())} events, "
          f"sha256 {hashlib.sha256(text.encode()).hexdigest()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
