"""The scheduler of the backward pass: which stream a weight / bias gradient is launched on, when parked tower gradients are released,
which launches share one hand-over to the side stream, what keeps their operands alive and when the main stream joins.  The op wrappers
(layers/functional.py) ask ``side_stream`` / ``batch_or_call`` per launch; all state lives in the one ``_Scheduler`` instance below."""
import ctypes
import os
import threading

import torch

from .._C import call


def at_end_of_backward(fn):
    """Queue ``fn`` on the autograd engine, to run when the backward pass that is executing has finished (not if it raises).
    -> False outside a backward pass: nothing was queued."""
    try:
        torch.autograd.Variable._execution_engine.queue_callback(fn)
    except RuntimeError:
        return False
    return True


def cu_mask_words(lo, hi, total=256):
    """Bit mask (list of 32-bit words) selecting the logical CUs lo .. hi-1 of hipExtStreamCreateWithCUMask's numbering.  On MI355X bit i
    lies on XCD i % 8, so a range whose ends are multiples of 8 takes the same number of CUs from every XCD (the workgroup -> XCD
    round-robin of a launch then still meets equally wide XCDs)."""
    words = [0] * ((total + 31) // 32)
    for i in range(max(0, lo), min(hi, total)):
        words[i // 32] |= 1 << (i % 32)
    return words


def make_stream(device, priority=0, role=None):
    """A side stream of the training step.  ``SOD_CUMASK_<ROLE>=lo:hi`` (role = WGRAD / TOWER / PREFETCH / MAIN) confines it to the
    logical compute units lo .. hi-1 (sod_stream_create_cumask; such a stream has the default priority); without the variable it is a
    plain torch stream of the given HIP priority."""
    spec = os.environ.get(f"SOD_CUMASK_{role}") if role else None
    if not spec:
        return torch.cuda.Stream(device=device, priority=priority)
    lo, hi = (int(v) for v in spec.split(":"))
    words = cu_mask_words(lo, hi)
    arr = (ctypes.c_uint * len(words))(*words)
    out = ctypes.c_void_p()
    with torch.cuda.device(device):
        call("sod_stream_create_cumask", ctypes.cast(arr, ctypes.c_void_p), len(words), ctypes.byref(out))
    return torch.cuda.ExternalStream(out.value, device=device)       # lives for the rest of the process


# Re-pairing the backward phases by roof (round 6; SOD_HOLD_HEAD_WGRAD=0 restores the old order).  The head towers' weight gradients are
# MFMA-bound, and so are the towers' data gradients they used to run beside (8.5 ms phase on three queues); the FPN / backbone backward
# that follows is HBM-bound on two saturated queues.  The tower units therefore PARK their weight-gradient launches (and the mark_ready
# behind them) and the first FPN / backbone backward node releases them, in order, onto the same side stream: they then run beside the
# HBM-bound kernels.  Same launches, same operands, same results; measured on the FCOS R50 step in alternating 60-step runs:
# 660.3 -> 665.3, 653.5 -> 661.7, 655.7 -> 660.8 img/s (+0.8 ... +1.2 %), one-rank RCCL rehearsal 646.5 -> 654.2 with the exposed
# communication unchanged (0.13 ms per step: the head's bucket is launched later, but 7 ms of backward are still ahead of it).  Releasing
# them onto a side stream of their OWN instead measured 14 % SLOWER (555 - 567 img/s at 4, 5 or 6 hardware queues): three streams of
# chip-filling kernels take each other's CUs; profiles/r6_pairing.txt.
HOLD_HEAD_WGRAD = os.environ.get("SOD_HOLD_HEAD_WGRAD", "1") != "0"

# False: one hand-over per weight-gradient launch (as until round 4).  Batching a whole residual block's weight gradients behind its data
# gradients measured SLOWER (623 vs 634 img/s, four alternating 100-step pairs, round 5: the side stream is the one that finishes last, and
# launches that reach it later lengthen the tail of backward by more than the bubbles save), so only launches that were adjacent anyway
# (weight + bias gradient of one convolution, conv1 + shortcut of a block) share a hand-over.
WGRAD_BATCH = True


class _Scheduler:
    """Weight gradients have no consumer until the optimizer (or the bucket all-reduce), while the data gradient of the same layer is on
    the critical path of backward.  Inside an autograd backward pass the wgrad launches therefore go to a per-device SIDE stream:
    the hardware interleaves the two queues, so the tail of one kernel's grid is filled by the other's workgroups.  The main stream
    joins the side stream in an end-of-backward callback (and the all-reduce stream waits for it per bucket, arena._launch_bucket).
    SOD_WGRAD_STREAM=0 (functional.WGRAD_SIDE_STREAM) keeps everything on one stream."""

    def __init__(self):
        self.sides = {}             # device index -> [side stream]
        self.keep = []              # operands of side-stream launches, referenced until the join
        self.join_queued = False    # the end-of-backward callback of the running backward pass is queued
        self.held = []              # parked launches of the tower units
        self.aux = {}               # device index -> extra streams that run backward nodes
        self.tls = threading.local()        # .items: the open batch of this thread; .flushing / .waited while it is issued

    # ---- end of backward
    def _in_backward(self):
        """True inside an autograd backward pass; the first call of a pass queues the join.  Parking and side-stream launches are only
        safe when something will release / join: op-level calls outside a backward pass launch at once on the current stream."""
        if not self.join_queued:
            self.join_queued = at_end_of_backward(self._end_of_backward)
        return self.join_queued

    def _end_of_backward(self):
        self.release_held()
        self._join_streams()

    def _join_streams(self):
        self.join_queued = False
        for idx, sides in self.sides.items():
            main = torch.cuda.current_stream(idx)
            for side in sides:
                main.wait_stream(side)
        self.keep.clear()       # the main stream now waits for every side-stream reader: the operands may go back to its pool

    def join(self):
        """Make the current stream(s) wait for every weight-gradient launch enqueued so far.  The end-of-backward callback does this
        on the normal path; the optimizer, the bucket reducer and zero_grad call it again so that a backward pass that ended in an
        exception (the callback never ran) leaves no gradient in flight.  Launches such a dead step left parked are DROPPED, never issued."""
        self.drop_held()
        self._join_streams()

    # ---- parked launches
    def hold_or_call(self, fn):
        """Tower units: run ``fn`` (weight-gradient launch + mark_ready) now, or park it until release_held()."""
        if HOLD_HEAD_WGRAD and self._in_backward():
            self.held.append(fn)
        else:
            fn()

    def release_held(self):
        """First FPN / backbone backward node (and the end-of-backward callback, at the latest): issue every parked launch, in order."""
        if self.held:
            items = list(self.held)
            self.held.clear()
            for fn in items:
                fn()

    def drop_held(self):
        """A backward pass that ended in an exception may leave parked launches behind: never carry them into the next step."""
        self.held.clear()

    # ---- batched hand-over to the side stream.  Every hand-over costs an event RECORD on the producing stream and a WAIT on the side
    # stream; the kernel trace prices each at 6-7 us of queue bubble (the next kernel of that queue starts that much later: 70 hand-overs
    # per FCOS step = 0.45 ms on the main queue and as much on the side queue, profiles/r5_step_occupancy.txt).  Inside
    # ``with wgrad_batch():`` the weight- / bias-gradient launches (and the arena.mark_ready calls that follow them) are collected and
    # issued together when the outermost block ends: ONE record + ONE wait for all of them.  A residual block's three or four weight
    # gradients then cost one hand-over instead of four.  A block that raises issues none of them.
    def batch_or_call(self, fn):
        """Run ``fn`` now, or behind the launches already collected in the open batch of this thread (arena.mark_ready: a bucket must
        not be handed to the reducer before the launches that fill it have been issued)."""
        items = getattr(self.tls, "items", None)
        if items is None or not WGRAD_BATCH:
            fn()
        else:
            items.append(fn)

    # ---- streams
    def side_stream(self, device, tensors):
        """Returns the stream to launch a wgrad on (None = current stream), ordered behind the current stream; ``tensors`` are the
        launch's operands.  (Launches that add to the same buffer always use the same stream: the slab / deterministic reductions
        update it with plain read-modify-writes.)"""
        if device.type != "cuda" or not self._in_backward():      # op-level calls: nobody would join, stay on the current stream
            return None
        sides = self.sides.get(device.index)
        if sides is None:
            # lowest HIP stream priority (range on MI355X: 1 .. -1): the data-gradient chain is the critical path.  Measured 491.5-492.3
            # (low) / 491.8 (normal) / 483-484 (high) img/s
            # (Two or three round-robin side streams measured neutral to worse in rounds 2 and 4 - 614.7 / 606 vs 613.8 img/s, 640.3 vs
            # 642.0 - and left the tree in round 5: one in-order side stream.)
            sides = self.sides[device.index] = [make_stream(device, 1, "WGRAD")]
        side = sides[0]
        # one wait per batch flush (the closures of a batch run back to back on this thread: nothing was enqueued on the current stream in
        # between, so the first launch's wait covers the others) - or one per launch outside a batch
        cur = torch.cuda.current_stream(device)
        if getattr(self.tls, "flushing", False):
            tag = (side.cuda_stream, cur.cuda_stream)
            if tag not in self.tls.waited:
                side.wait_stream(cur)
                self.tls.waited.add(tag)
        else:
            side.wait_stream(cur)
        # The operands (dY, X) must outlive the side-stream kernel.  They are kept referenced until the join instead of
        # Tensor.record_stream(): with record_stream the allocator cannot reuse a block until a GPU-side event has completed, and since the
        # host runs several steps ahead of the GPU the pool grew from 10 GB to 52 GB; held references are released in main-stream order
        # right after the join is enqueued, so the pool stays at its single-stream size plus one backward pass of gradients.
        self.keep.extend(t for t in tensors if t is not None)
        return side

    def wgrad_side_streams(self, device):
        """The side streams of ``device`` on which wgrad work may be pending in this backward pass (empty list if none)."""
        return list(self.sides.get(device.index, ())) if self.join_queued else []

    def register_compute_stream(self, device, stream):
        """Announce an extra stream that runs backward nodes (e.g. the FCOS box tower's).  Parameter gradients may be produced on it, so
        the bucket reducer (arena._launch_bucket) waits for it in addition to the launching node's stream and the wgrad side stream."""
        lst = self.aux.setdefault(device.index, [])
        if all(s.cuda_stream != stream.cuda_stream for s in lst):
            lst.append(stream)

    def aux_compute_streams(self, device):
        return list(self.aux.get(device.index, ()))


sched = _Scheduler()
side_stream, join = sched.side_stream, sched.join
hold_or_call, release_held, drop_held, batch_or_call = sched.hold_or_call, sched.release_held, sched.drop_held, sched.batch_or_call
wgrad_side_streams, register_compute_stream, aux_compute_streams = sched.wgrad_side_streams, sched.register_compute_stream, sched.aux_compute_streams


class wgrad_batch:
    """``with wgrad_batch():`` - see _Scheduler.batch_or_call.  Nested blocks flush at the outermost exit, in order."""

    def __enter__(self):
        self.outer = getattr(sched.tls, "items", None)
        if self.outer is None:
            sched.tls.items = []
        return self

    def __exit__(self, et, ev, tb):
        if self.outer is None:
            items, sched.tls.items = sched.tls.items, None
            if et is None and items:
                sched.tls.flushing, sched.tls.waited = True, set()      # side_stream: one wait per (side, current) pair from here on
                try:
                    for fn in items:
                        fn()
                finally:
                    sched.tls.flushing, sched.tls.waited = False, None
        return False
