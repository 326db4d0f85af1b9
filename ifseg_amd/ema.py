"""The teacher of the self-training path: an exponential moving average of the trainable arena.

Specification (this module) and state of what `Trainer(store_ema=True)` keeps.  The rule is fairseq's
`EMA._step_internal` (fairseq/models/ema/ema.py:134-167) with `ema_fp32=True` on a 16-bit model, element for element:

    ema.mul_(decay); ema.add_(param.float(), alpha=1 - decay)

* the source is the ROUNDED bf16 model weight (`model.state_dict()`), not the fp32 master of the optimizer;
* the two lines are a rounded product followed by ONE fused multiply-add (ATen's `add_(alpha=)` is an fma per element):

    d32 = float32(decay)        r32 = float32(1.0 - decay)      (the subtraction in double, as Python does it)
    u   = round32(e * d32)
    e'  = fma(r32, float(p16), u)                               (rounded once)
    e16 = bf16_rne(e')

  decay == 0 is fairseq's copy phase before `ema_start_update`: e' = float(p16).

On the device the rule is the epilogue of the optimizer launch (`hip.adam_ema_step`, csrc/optim.hip): the new bf16 weight is
in registers there.  Not built: a stand-alone EMA launch (nothing here would call it) -- `ArenaEMA.update` exists on the CPU
only, where it runs this specification.
"""
import torch


def ema_scalars(decay):
    """(d32, r32) as Python floats that hold float32 values: what the kernel is handed and what the specification uses"""
    d = torch.tensor(float(decay), dtype=torch.float64)
    return float(d.float()), float((1.0 - d).float())


def _fma32(a, b, c):
    """float32 fma(a, b, c) of CPU tensors where a * b is exact in float64 (b: one float32 scalar, a: bf16 values cast up):
    the float64 sum, rounded to odd with the error of the addition, then rounded to float32 -- independent of whether the
    ATen build at hand contracts, vectorises or handles its scalar tail differently"""
    prod = a.double() * b
    c = c.double()
    s = c + prod
    bb = s - c                                             # TwoSum: err is the exact rounding error of s
    err = (c - (s - bb)) + (prod - bb)
    bits = s.view(torch.int64).clone()
    inexact = (err != 0) & torch.isfinite(s) & torch.isfinite(err)
    even = (bits & 1) == 0
    away = (err > 0) == (s > 0)                            # the exact sum lies further from zero than s
    bits = torch.where(inexact & even, torch.where(away, bits + 1, bits - 1), bits)
    return bits.view(torch.float64).float()


def ema_reference(e32, p16, decay):
    """-> (e32', e16'): one EMA step of fp32 `e32` towards bf16 `p16` (CPU tensors, nothing is modified)"""
    if e32.dtype != torch.float32 or p16.dtype != torch.bfloat16 or e32.shape != p16.shape:
        raise ValueError("ema_reference: e32 fp32 and p16 bf16 of one shape, got %s %s and %s %s"
                         % (e32.dtype, tuple(e32.shape), p16.dtype, tuple(p16.shape)))
    d32, r32 = ema_scalars(decay)
    u = e32 * torch.tensor(d32, dtype=torch.float32)
    out = _fma32(p16.float(), r32, u)
    return out, out.to(torch.bfloat16)


def ema_decay_at(updates, decay, start_update):
    """fairseq's `EMA.step`: the decay of the EMA step that follows update number `updates` (the count AFTER the update, as
    trainer.py:962-969 passes it): 0.0 -- a copy -- while updates < start_update"""
    return 0.0 if updates < start_update else float(decay)


def check_arenas(what, p32, p16, e32, e16):
    """student and teacher arenas of one exchange: dtypes, one length, contiguous, no overlap; ValueError names the culprit"""
    for name, t, dt in (("p32", p32, torch.float32), ("p16", p16, torch.bfloat16), ("e32", e32, torch.float32),
                        ("e16", e16, torch.bfloat16)):
        if not torch.is_tensor(t) or t.dtype != dt:
            raise ValueError("%s: %s must be a %s tensor, got %s" % (what, name, dt, getattr(t, "dtype", type(t))))
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s: %s must be a flat contiguous arena" % (what, name))
        if t.device != p32.device:
            raise ValueError("%s: %s is on %s, p32 on %s" % (what, name, t.device, p32.device))
    n = p32.numel()
    for name, t in (("p16", p16), ("e32", e32), ("e16", e16)):
        if t.numel() != n:
            raise ValueError("%s: %s has %d elements, p32 has %d" % (what, name, t.numel(), n))
    spans = [(name, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
             for name, t in (("p32", p32), ("p16", p16), ("e32", e32), ("e16", e16))]
    for i, (na, a0, a1) in enumerate(spans):
        for nb, b0, b1 in spans[i + 1:]:
            if a0 < b1 and b0 < a1:
                raise ValueError("%s: %s and %s overlap" % (what, na, nb))
    return n


class ArenaEMA:
    """fp32 teacher `e32` and its bf16 rounding `e16` beside a student's arenas `p32` (fp32 masters, [n_train]) and `p16` (the
    first n_train elements of the bf16 parameter arena), with fairseq's schedule (`ema_decay`, `ema_start_update`,
    `ema_update_freq`, EMAConfig's names).  The arenas live where `p32` lives; on the CPU every operation is this module's
    specification, on the device the step is `hip.adam_ema_step`'s (issued by the Trainer) and the swap `hip.ema_swap`'s.
    `device` only states where the caller expects them (as augment.py's and artificial.py's `device="cpu"`)."""

    def __init__(self, p32, p16, decay=0.9999, start_update=0, update_freq=1, device=None):
        if device is not None and torch.is_tensor(p32) and torch.device(device).type != p32.device.type:
            raise ValueError("ArenaEMA: device %s, but the arenas live on %s" % (device, p32.device))
        self.e32, self.e16 = torch.empty_like(p32), torch.empty_like(p16)
        self.n = check_arenas("ArenaEMA", p32, p16, self.e32, self.e16)
        if not 0.0 <= float(decay) <= 1.0 or int(update_freq) < 1:
            raise ValueError("ArenaEMA: ema_decay in [0, 1] and ema_update_freq >= 1, got %r and %r" % (decay, update_freq))
        self.p32, self.p16 = p32, p16
        self.decay, self.start_update, self.update_freq = float(decay), int(start_update), int(update_freq)
        self.counter = 0                # fairseq's update_freq_counter
        self.last_decay = self.decay    # EMA.get_decay()
        self.swapped = False
        self.seed()

    @property
    def device(self):
        return self.p32.device

    def seed(self):
        """teacher := student.  `fresh` stays set until a step or a load has touched the teacher (the Trainer clears it when it
        re-seeds in front of its first optimizer launch)"""
        self.e32.copy_(self.p32)
        self.e16.copy_(self.p16)
        self.fresh = True

    def schedule(self, updates):
        """fairseq's `EMA.step` for the update that brings the count to `updates`: advances the frequency counter and returns
        (d32, r32) of the EMA step to take with it, or None on an off-update of `ema_update_freq`"""
        self.last_decay = ema_decay_at(updates, self.decay, self.start_update)
        if self.update_freq > 1:
            self.counter += 1
            if self.counter < self.update_freq:
                return None
            self.counter = 0
        return ema_scalars(self.last_decay)

    def update(self, updates):
        """CPU only: the step the fused optimizer launch takes on the device"""
        if self.device.type != "cpu":
            raise RuntimeError("ArenaEMA.update: on the device the step is part of hip.adam_ema_step (no stand-alone launch)")
        dr = self.schedule(updates)
        if dr is not None:
            self.fresh = False
            e32, e16 = ema_reference(self.e32, self.p16, self.last_decay)
            self.e32.copy_(e32)
            self.e16.copy_(e16)
        return dr

    def swap(self):
        """student <-> teacher, in place, both precisions"""
        if self.device.type == "cpu":
            check_arenas("ArenaEMA.swap", self.p32, self.p16, self.e32, self.e16)
            for a, b in ((self.p32, self.e32), (self.p16, self.e16)):
                t = a.clone()
                a.copy_(b)
                b.copy_(t)
        else:
            from . import hip
            hip.ema_swap(self.p32, self.p16, self.e32, self.e16)
        self.swapped = not self.swapped

    def state_dict(self):
        if self.swapped:
            raise RuntimeError("ArenaEMA.state_dict: student and teacher are swapped")
        return {"e32": self.e32.clone(), "counter": self.counter, "last_decay": self.last_decay}

    def load_state_dict(self, sd):
        if self.swapped:
            raise RuntimeError("ArenaEMA.load_state_dict: student and teacher are swapped")
        e32 = sd["e32"]
        if not torch.is_tensor(e32) or e32.dtype != torch.float32 or e32.numel() != self.n:
            raise ValueError("ArenaEMA.load_state_dict: e32 must be fp32 with %d elements" % self.n)
        self.e32.copy_(e32.reshape(-1))
        self.e16.copy_(self.e32)                            # RNE: what the kernel's epilogue stores
        self.counter, self.last_decay = int(sd.get("counter", 0)), float(sd.get("last_decay", self.decay))
        self.fresh = False
