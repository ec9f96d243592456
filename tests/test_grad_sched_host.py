"""The backward scheduler (layers/grad_sched.py) with toy CPU autograd nodes: what is parked, batched and released, in which order,
and what survives a backward pass that raised.  No GPU, no native library: the nodes' backwards only append to a log through the
scheduler's calls; the stream bookkeeping is checked with fake streams in place of torch's."""
import types

import pytest
import torch

from slenderobjdet_amd.layers import grad_sched as GS

STEP_LOG = ["tower-dgrad", "held-wgrad", "inside-batch", "w", "mark", "fpn-dgrad"]


class _Node(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, body):
        ctx.body = body
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.body()
        return g, None


def _backward(*bodies):
    """One backward pass over a chain of nodes; ``bodies`` are given in the order their backwards run."""
    y = torch.zeros(1, requires_grad=True)
    for body in reversed(bodies):
        y = _Node.apply(y, body)
    y.sum().backward()


@pytest.fixture(autouse=True)
def fresh_scheduler(monkeypatch):
    GS.sched.__init__()
    monkeypatch.setattr(GS, "HOLD_HEAD_WGRAD", True)
    monkeypatch.setattr(GS, "WGRAD_BATCH", True)
    yield
    GS.sched.__init__()


def _tower(log):
    def body():
        log.append("tower-dgrad")
        GS.hold_or_call(lambda: log.append("held-wgrad"))
    return body


def _fpn(log):
    def body():
        GS.release_held()
        with GS.wgrad_batch():
            GS.batch_or_call(lambda: log.append("w"))
            log.append("inside-batch")
            GS.batch_or_call(lambda: log.append("mark"))
        log.append("fpn-dgrad")
    return body


def _idle():
    return not GS.sched.held and not GS.sched.join_queued and not GS.sched.keep


def test_hold_or_call_outside_backward_runs_at_once():
    log = []
    GS.hold_or_call(lambda: log.append("now"))
    assert log == ["now"] and _idle()


def test_parked_launch_is_released_by_the_next_node_and_batches_flush_in_order():
    log = []
    _backward(_tower(log), _fpn(log))
    assert log == STEP_LOG and _idle()


def test_nested_batches_flush_at_the_outermost_exit():
    log = []
    with GS.wgrad_batch():
        GS.batch_or_call(lambda: log.append("a"))
        with GS.wgrad_batch():
            GS.batch_or_call(lambda: log.append("b"))
        log.append("inner-closed")
        GS.batch_or_call(lambda: log.append("c"))
        log.append("body-done")
    assert log == ["inner-closed", "body-done", "a", "b", "c"]
    GS.batch_or_call(lambda: log.append("after"))       # no batch open any more
    assert log[-1] == "after"


def test_batch_whose_body_raises_runs_none_of_its_items():
    log = []
    with pytest.raises(ValueError):
        with GS.wgrad_batch():
            GS.batch_or_call(lambda: log.append("a"))
            with GS.wgrad_batch():
                GS.batch_or_call(lambda: log.append("b"))
            raise ValueError("body")
    assert log == []
    GS.batch_or_call(lambda: log.append("after"))       # and the batch is closed
    assert log == ["after"]


def test_batching_switched_off_runs_items_immediately(monkeypatch):
    monkeypatch.setattr(GS, "WGRAD_BATCH", False)
    log = []
    with GS.wgrad_batch():
        GS.batch_or_call(lambda: log.append("a"))
        log.append("body")
    assert log == ["a", "body"]


def test_without_a_release_point_parked_launches_run_at_end_of_backward():
    log = []
    _backward(_tower(log), lambda: log.append("other-dgrad"))
    assert log == ["tower-dgrad", "other-dgrad", "held-wgrad"] and _idle()


def test_holding_switched_off_runs_immediately(monkeypatch):
    monkeypatch.setattr(GS, "HOLD_HEAD_WGRAD", False)
    log = []
    _backward(_tower(log), lambda: log.append("other-dgrad"))
    assert log == ["tower-dgrad", "held-wgrad", "other-dgrad"] and _idle()


def test_at_end_of_backward_queues_once_per_pass():
    log, queued = [], []
    assert GS.at_end_of_backward(lambda: log.append("never")) is False
    _backward(lambda: queued.append(GS.at_end_of_backward(lambda: log.append("end"))), lambda: log.append("dgrad"))
    assert queued == [True] and log == ["dgrad", "end"]
    _backward(lambda: log.append("next-pass"))          # the callback belonged to the first pass only
    assert log == ["dgrad", "end", "next-pass"]


def test_failed_backward_leaves_nothing_for_the_next_step():
    log = []

    def failing():
        raise RuntimeError("boom")

    with pytest.raises(RuntimeError, match="boom"):
        _backward(_tower(log), failing)
    assert log == ["tower-dgrad"]
    GS.join()                                           # what the optimizer, finish_backward and zero_grad call
    assert log == ["tower-dgrad"] and _idle()           # the dead step's launch was dropped, not issued
    GS.hold_or_call(lambda: log.append("op-level"))
    assert log == ["tower-dgrad", "op-level"]
    del log[:]
    _backward(_tower(log), _fpn(log))
    assert log == STEP_LOG and _idle()


class _FakeStream:
    def __init__(self, handle, waits):
        self.cuda_stream, self.waits = handle, waits

    def wait_stream(self, other):
        self.waits.append((self.cuda_stream, other.cuda_stream))


def test_side_launches_of_one_batch_flush_share_one_wait(monkeypatch):
    waits, made = [], []
    main, dev = _FakeStream(1, waits), types.SimpleNamespace(type="cuda", index=0)

    def make_stream(device, priority, role):
        made.append((device.index, priority, role))
        return _FakeStream(2, waits)

    monkeypatch.setattr(GS, "make_stream", make_stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: main)
    assert GS.side_stream(dev, ["dy"]) is None and not waits and not made         # outside a backward pass: the current stream
    assert GS.side_stream(types.SimpleNamespace(type="cpu", index=None), []) is None
    got = []

    def batched():
        with GS.wgrad_batch():
            for i in range(3):
                GS.batch_or_call(lambda i=i: got.append(GS.side_stream(dev, [f"dy{i}", None])))
        assert waits == [(2, 1)] and GS.sched.keep == ["dy0", "dy1", "dy2"]
        assert [s.cuda_stream for s in GS.wgrad_side_streams(dev)] == [2]

    def single():
        for i in range(3):
            got.append(GS.side_stream(dev, [f"x{i}"]))
        assert waits == [(2, 1)] * 4

    _backward(batched, single)
    assert made == [(0, 1, "WGRAD")] and all(s.cuda_stream == 2 for s in got) and len(got) == 6
    assert waits == [(2, 1)] * 4 + [(1, 2)] and _idle()      # the end-of-backward join: main waits for the side stream
    assert GS.wgrad_side_streams(dev) == []
