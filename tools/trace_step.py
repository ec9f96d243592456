"""Launch trace of one training step: the sequence of library entry points with the stream each was launched on, and of the waits
between streams, for FCOS, RetinaNet, RepPoints (DeformConv) and the rotated two-stage model at test sizes (R18, 2 images).

    python tools/trace_step.py [--arch fcos retinanet ...] [--steps 2] [--out FILE]

Only the loaded library object (_C._lib) and torch.cuda.Stream.wait_stream / wait_event / Event.record are wrapped, so the same file
runs in any checkout: two revisions schedule the backward pass identically iff their outputs are equal line for line (diff them; also
with SOD_WGRAD_STREAM=0 SOD_HOLD_HEAD_WGRAD=0).  Streams and events are numbered by first appearance."""
import argparse
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from slenderobjdet_amd import _C
from slenderobjdet_amd.data import synthetic_batch
from slenderobjdet_amd.modeling import build_model
from slenderobjdet_amd.solver import build_optimizer

SIZES = {"fcos": (320, 384), "retinanet": (256, 320), "reppoints": (192, 256), "rrcnn": (256, 320)}


class Recorder:
    def __init__(self):
        self.lines, self.streams, self.events = [], {}, {}

    def stream(self, handle):
        return "s%d" % self.streams.setdefault(handle or 0, len(self.streams))

    def event(self, ev):
        return "e%d" % self.events.setdefault(id(ev), (len(self.events), ev))[0]      # (the event is kept: no id is reused within a step)

    def reset(self):
        self.lines, self.events = [], {}        # stream numbers persist: a stream is the same queue in every step


REC = Recorder()


class LibProxy:
    """Stands in for the ctypes library: every entry point is recorded with the stream it was given - by convention the last
    argument, taken as a stream when it is NULL, the current stream, or a stream already seen in a wait / record."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def wrapper(*args):
            where = "-"
            if args and isinstance(args[-1], ctypes.c_void_p):
                handle = args[-1].value or 0
                if handle in REC.streams or handle == torch.cuda.current_stream().cuda_stream:
                    where = REC.stream(handle)
            REC.lines.append(f"L {name} {where}")
            return fn(*args)
        return wrapper


def patch():
    _C.load()
    _C._lib = LibProxy(_C._lib)
    wait_stream, wait_event, record = torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record

    def rec_wait_stream(self, other):
        REC.lines.append(f"W wait_stream {REC.stream(self.cuda_stream)} <- {REC.stream(other.cuda_stream)}")
        return wait_stream(self, other)

    def rec_wait_event(self, event):
        REC.lines.append(f"W wait_event {REC.stream(self.cuda_stream)} <- {REC.event(event)}")
        return wait_event(self, event)

    def rec_record(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        REC.lines.append(f"W record {REC.event(self)} on {REC.stream(s.cuda_stream)}")
        return record(self, stream)

    torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record = rec_wait_stream, rec_wait_event, rec_record


def trace(arch, steps):
    cfg = bench.make_cfg(18, arch, constant_lr=True)
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    if arch in ("retinanet", "rrcnn"):
        bench.damp_residual_branches(model)
    opt = build_optimizer(cfg, model)
    h, w = SIZES[arch]
    data = synthetic_batch(2, h, w, 3, device="cuda", rotated=arch == "rrcnn")
    REC.stream(torch.cuda.current_stream().cuda_stream)
    out, params = [], model.arena.params.detach().clone()
    for step in range(steps):
        REC.reset()
        bench.train_step(model, opt, data)
        torch.cuda.synchronize()
        with torch.no_grad():       # every step from the same weights: the two-stage model's launches depend on its proposals, and the
            model.arena.params.copy_(params)        # update of a step on float atomics that differ from run to run
        out += [f"{arch} step{step} {line}" for line in REC.lines]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--steps", type=int, default=2, help="the first step also creates the side streams; the second is the steady state")
    ap.add_argument("--out", help="write the trace here instead of printing it (the digests are always printed)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    patch()
    lines = []
    for arch in args.arch:
        got = trace(arch, args.steps)
        print(f"# {arch}: {len(got)} lines, sha1 {hashlib.sha1(chr(10).join(got).encode()).hexdigest()}", flush=True)
        lines += got
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
