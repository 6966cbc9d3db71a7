"""`--against OTHER.so` of the rate tools (separation_rate.py, conflicts_rate.py, flown_separation_rate.py, flown_conflicts_rate.py, plan_audit_rate.py, retime_rate.py): the
gate of a change to a kernel that must not change a bit nor cost time.  The same calls through this build (lib/libuavac.so, or the one
UAVAC_LIB names) and through another build of the same ABI (the parent commit's, say), both loaded privately into one process (RTLD_LOCAL,
and RTLD_DEEPBIND: a library's calls into itself stay in it even where the tool has made its inputs through `uav_ac`, which loads this
build RTLD_GLOBAL) and called through ctypes alone; on the same inputs, alternating which goes first.
The two builds' outputs are compared byte for byte BEFORE anything is timed, and a difference ends the run.  Per build one JSON line: the
times of every round, their median and spread, and the ratio of the two medians.  Run it with a byte-identical copy of one library as
OTHER.so to see what ratio this method gives to no difference at all."""
import ctypes as C
import json
import os
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p
THIS, OTHER = "this build", "the other build"


def ptr(t):
    return None if t is None else P(t.data_ptr())


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


class Builds:
    def __init__(self, other, argtypes):
        """`argtypes` {entry point: its argument types} of what the tool calls, besides create / set_stream / device_identity."""
        self.paths = {THIS: os.environ.get("UAVAC_LIB") or os.path.join(ROOT, "uav-autonomous-control_amd", "lib", "libuavac.so"),
                      OTHER: os.path.abspath(other)}
        torch.cuda.set_device(0)
        self.lib, self.ctx = {}, {}
        for name, path in self.paths.items():
            lib = C.CDLL(path, mode=C.RTLD_LOCAL | os.RTLD_DEEPBIND)
            lib.uavac_create.argtypes = [C.POINTER(P), C.c_int]
            lib.uavac_set_stream.argtypes = [P, P]
            lib.uavac_device_identity.argtypes = [P, C.c_char_p, C.c_int]
            for fn, types in argtypes.items():
                getattr(lib, fn).argtypes = types
            h = P()
            assert lib.uavac_create(C.byref(h), 0) == 0
            assert lib.uavac_set_stream(h, P(torch.cuda.current_stream().cuda_stream or None)) == 0
            self.lib[name], self.ctx[name] = lib, h
        ident = C.create_string_buffer(256)
        self.lib[THIS].uavac_device_identity(self.ctx[THIS], ident, 256)
        self.box = ident.value.decode(errors="replace")
        self.lines = []

    def alternate(self, arm, call, rounds, reps=5, **meta):
        """`call(lib, ctx)` -> the tensors one call wrote.  Warm-up, the byte-for-byte comparison, then `rounds` rounds of `reps` calls
        per build, the build that goes first alternating."""
        out = {name: call(self.lib[name], self.ctx[name]) for name in self.lib}
        torch.cuda.synchronize()
        for a, b in zip(out[THIS], out[OTHER]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), \
                f"{arm}: the two builds' outputs differ"
        ms = {name: [] for name in self.lib}
        for rnd in range(rounds):
            for name in (list(self.lib) if rnd % 2 == 0 else list(self.lib)[::-1]):
                ms[name].append(timed(lambda: call(self.lib[name], self.ctx[name]), reps))
        for name, ts in ms.items():
            med = float(np.median(ts))
            self.lines.append(json.dumps({"arm": f"{arm}, {name}, alternating with the other", "library": os.path.relpath(self.paths[name], ROOT),
                                          **meta, "ms_per_round": [round(t, 4) for t in ts], "median_ms": round(med, 4),
                                          "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                                          "spread (max - min) / median": round((max(ts) - min(ts)) / med, 5), "rounds": rounds,
                                          "median / the other build's median": round(med / float(np.median(ms[OTHER])), 5),
                                          "outputs of the two builds agree": True, "box": self.box}))
            print(self.lines[-1], flush=True)

    def wall(self, arm, call, rounds, **meta):
        """`alternate` for calls that return to the host (the twins, N back-to-back calls): `call(lib, ctx)` -> the arrays one call wrote
        (NumPy or tensors); wall-clock seconds per call and round, the device drained before and after."""
        got = {}
        for name in self.lib:
            got[name] = [np.array(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in call(self.lib[name], self.ctx[name])]
            torch.cuda.synchronize()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[THIS], got[OTHER])), f"{arm}: the two builds' outputs differ"
        sec = {name: [] for name in self.lib}
        for rnd in range(rounds):
            for name in (list(self.lib) if rnd % 2 == 0 else list(self.lib)[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(self.lib[name], self.ctx[name])
                torch.cuda.synchronize()
                sec[name].append(time.perf_counter() - t0)
        for name, ts in sec.items():
            med = float(np.median(ts))
            self.lines.append(json.dumps({"arm": f"{arm}, {name}, alternating with the other", "library": os.path.relpath(self.paths[name], ROOT),
                                          **meta, "ms_per_round": [round(t * 1e3, 4) for t in ts], "median_ms": round(med * 1e3, 4),
                                          "rounds": rounds, "median / the other build's median": round(med / float(np.median(sec[OTHER])), 5),
                                          "outputs of the two builds agree": True, "box": self.box}))
            print(self.lines[-1], flush=True)

    def write(self, out_path):
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as fh:
                fh.write("\n".join(self.lines) + "\n")


def split_argv(argv):
    """-> (argv without the option, OTHER.so or None)"""
    argv = list(argv)
    other = None
    if "--against" in argv:
        at = argv.index("--against")
        other = argv[at + 1]
        del argv[at:at + 2]
    return argv, other
