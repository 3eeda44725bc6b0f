"""Device-side step telemetry: a ring of (loss, gradient sum of squares) records that
``mdemi_telemetry_push`` (csrc/telemetry.hip) appends once per optimizer step, on the
step's own stream -- inside the captured hipGraph in graph mode -- and that the host
reads with one copy every ``train.print_freq`` steps (train.loop.fit).  Nothing here
synchronises per step.  The push also flags a non-finite loss or gradient norm.  Under the
default policy (train.nonfinite: "stop") the unguarded AdamW kernels have already written
such a step into the weights and the driver stops instead of checkpointing them; under
"skip" the guarded update dropped it on the same scalar and the same predicate, so a record
flagged MDEMI_STEP_GRAD_NONFINITE is a skipped step."""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np
import torch

from .. import _lib as L

StepRecord = namedtuple("StepRecord", "loss grad_sumsq index flags")
Drained = namedtuple("Drained", "records dropped pushed")

_STATE_BYTES = ctypes.sizeof(L.TelemetryState)
_REC_DTYPE = np.dtype(L.StepRecord)  # the fields of mdemi_step_record, as the header declares them
assert _REC_DTYPE.itemsize == ctypes.sizeof(L.StepRecord) == 16 and _STATE_BYTES == 16


class NonFiniteStep(RuntimeError):
    """A recorded step had a non-finite loss or gradient norm; ``first_index`` is the
    0-based index (push count) of the first one, ``count`` how many there were."""

    def __init__(self, first_index, count=1):
        super().__init__(f"non-finite loss or gradient norm first seen at recorded step {first_index} "
                         f"({count} such step(s))")
        self.first_index, self.count = int(first_index), int(count)


def decode_ring(records, pushed, last_seen, capacity):
    """The records with index last_seen .. pushed-1 that a ring of ``capacity`` slots still
    holds, oldest first, and how many were overwritten before they were read.

    records: the ring in slot order (record i lives in slot i % capacity), each with an
    ``index`` field (attribute or key); pushed: records appended so far; last_seen: the
    value of ``pushed`` at the previous drain.  Returns (list, dropped)."""
    capacity, pushed, last_seen = int(capacity), int(pushed), int(last_seen)
    if capacity <= 0 or len(records) != capacity:
        raise ValueError(f"decode_ring: {len(records)} slots for capacity {capacity}")
    if not 0 <= last_seen <= pushed:
        raise ValueError(f"decode_ring: last_seen {last_seen} outside [0, pushed={pushed}]")
    new = pushed - last_seen
    kept = min(new, capacity)
    out = []
    for idx in range(pushed - kept, pushed):
        r = records[idx % capacity]
        got = r.index if isinstance(r, tuple) else r["index"]  # a StepRecord, or a dict / numpy record
        if int(got) != idx:
            raise ValueError(f"decode_ring: slot {idx % capacity} holds record {int(got)}, expected {idx}")
        out.append(r)
    return out, new - kept


class Telemetry:
    """Owns the device ring and its counters.  push() is one kernel launch; drain() is one
    device-to-host copy of the counters and the ring."""

    def __init__(self, capacity=1024, device=None):
        if int(capacity) <= 0:
            raise ValueError("Telemetry: capacity must be positive")
        self.capacity = int(capacity)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        L.load()
        host = torch.zeros(_STATE_BYTES + 16 * self.capacity, dtype=torch.uint8)
        host[:_STATE_BYTES].view(torch.int32).copy_(torch.tensor([0, 0, -1, 0], dtype=torch.int32))
        self._buf = host.to(self.device)  # [mdemi_telemetry_state | mdemi_step_record x capacity]
        self._last_seen = 0

    @property
    def state_ptr(self):
        return self._buf.data_ptr()

    @property
    def ring_ptr(self):
        return self._buf.data_ptr() + _STATE_BYTES

    def push(self, loss_tensor, optimizer=None):
        """Append (loss, optimizer.grad_sumsq_tensor()) on the current stream.  optimizer None
        (or one without grad_sumsq_tensor): the record's grad_sumsq is -1."""
        if not (loss_tensor.is_cuda and loss_tensor.dtype == torch.float32 and loss_tensor.numel() == 1):
            raise ValueError("Telemetry.push: the loss must be a one-element fp32 CUDA tensor")
        gsq = optimizer.grad_sumsq_tensor() if hasattr(optimizer, "grad_sumsq_tensor") else None
        L.check(L.load().mdemi_telemetry_push(self.ring_ptr, self.capacity, self.state_ptr, loss_tensor.data_ptr(),
                                              L.ptr(gsq), L.stream()), "telemetry_push")

    def snapshot(self):
        """(state dict, ring as a numpy record array in slot order): one D2H copy."""
        raw = self._buf.cpu().numpy()
        st = raw[:_STATE_BYTES].view("<i4")
        state = {"pushed": int(st[0]), "nonfinite_steps": int(st[1]), "first_nonfinite": int(st[2])}
        return state, raw[_STATE_BYTES:].view(_REC_DTYPE)

    def drain(self, raise_on_nonfinite=True):
        """Drained(records, dropped, pushed): the StepRecords pushed since the last drain, in
        order; ``dropped`` counts those overwritten because more than ``capacity`` arrived in
        between.  Raises NonFiniteStep when any recorded step was flagged;
        raise_on_nonfinite=False returns the flagged records with the others instead (their
        ``flags`` say which), for a caller that handles them."""
        state, ring = self.snapshot()
        if raise_on_nonfinite and state["nonfinite_steps"] > 0:
            raise NonFiniteStep(state["first_nonfinite"], state["nonfinite_steps"])
        recs, dropped = decode_ring(ring, state["pushed"], self._last_seen, self.capacity)
        self._last_seen = state["pushed"]
        out = [StepRecord(float(r["loss"]), float(r["grad_sumsq"]), int(r["index"]), int(r["flags"])) for r in recs]
        return Drained(out, dropped, state["pushed"])
