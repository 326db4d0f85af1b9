"""CPU: the specification of the teacher (ifseg_amd/ema.py) against fairseq's own two lines and, where the reference's vendored
fairseq is importable, against its `EMA` class; `ArenaEMA` on the CPU (schedule, swap, state dict, refusals); the surface
(header, ABI version, bindings, Trainer keywords)."""
import importlib.util
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAYS = (0.0, 0.5, 0.999, 0.9999)


def arenas(n, seed, wide=False):
    """(e32, p16): normal values, with `wide` over sixty orders of magnitude and with zeros of both signs and subnormals"""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(n, generator=g)
    p = torch.randn(n, generator=g)
    if wide:
        e = e * torch.exp(torch.randn(n, generator=g) * 20).clamp(1e-30, 1e30)
        p = p * torch.exp(torch.randn(n, generator=g) * 20).clamp(1e-30, 1e30)
        special = torch.tensor([0.0, -0.0, 1e-39, -3e-40, 1e30, -1e30, 1e-30, 1.0])
        k = min(n, special.numel())
        e[:k] = special[:k]
        p[n - k:] = special[:k]
    return e, p.to(torch.bfloat16)


@pytest.mark.parametrize("n", [1, 7, 1027])
@pytest.mark.parametrize("decay", DECAYS)
def test_reference_is_fairseqs_two_lines(n, decay):
    """fairseq/models/ema/ema.py:164-165 on a float32 `ema_param` and a bf16 `param`, bit for bit"""
    from ifseg_amd.ema import ema_reference
    for wide in (False, True):
        e, p = arenas(n, 100 * n + int(decay * 10000), wide)
        want = e.clone()
        want.mul_(decay)
        want.add_(p.to(dtype=want.dtype), alpha=1 - decay)
        keep_e, keep_p = e.clone(), p.clone()
        got32, got16 = ema_reference(e, p, decay)
        assert torch.equal(got32.view(torch.int32), want.view(torch.int32))
        assert got16.dtype == torch.bfloat16 and torch.equal(got16.view(torch.int16), got32.to(torch.bfloat16).view(torch.int16))
        assert torch.equal(e.view(torch.int32), keep_e.view(torch.int32)) and torch.equal(p.view(torch.int16), keep_p.view(torch.int16))
        if decay == 0.0:
            assert torch.equal(got32, p.float())            # the copy phase (as values: -0 + +0 is +0)


def test_decay_schedule():
    from ifseg_amd.ema import ema_decay_at, ema_scalars
    assert [ema_decay_at(u, 0.99, 2) for u in (0, 1, 2, 3)] == [0.0, 0.0, 0.99, 0.99]
    assert ema_decay_at(1, 0.5, 0) == 0.5
    d, r = ema_scalars(0.9999)
    assert d == float(torch.tensor(0.9999, dtype=torch.float32)) and r == float(torch.tensor(1.0 - 0.9999, dtype=torch.float32))
    assert ema_scalars(0.0) == (0.0, 1.0)


CHILD = r'''
import os, sys
ROOT, SHIM = sys.argv[1], sys.argv[2] == "1"
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, ROOT)
if SHIM:
    import _refshim
    _refshim.install()
import torch
from types import SimpleNamespace
from fairseq.models.ema import EMA
from ifseg_amd.ema import ArenaEMA
torch.manual_seed(3)
lin = torch.nn.Linear(37, 5).to(torch.bfloat16)
cfg = SimpleNamespace(ema_decay=0.99, ema_start_update=2, ema_update_freq=2, ema_fp32=True, ema_seed_model=None)
ema = EMA(lin, cfg)
flat = lambda sd: torch.cat([sd["weight"].reshape(-1), sd["bias"].reshape(-1)])
p16 = flat(lin.state_dict()).clone()
mine = ArenaEMA(p16.float(), p16, decay=0.99, start_update=2, update_freq=2)
g = torch.Generator().manual_seed(4)
stepped = 0
for updates in range(1, 7):
    with torch.no_grad():
        for p in lin.parameters():
            p.add_((torch.randn(p.shape, generator=g) * 0.1).to(torch.bfloat16))
    ema.step(lin, updates)
    p16.copy_(flat(lin.state_dict()))
    stepped += mine.update(updates) is not None
    assert mine.last_decay == ema.get_decay(), (updates, mine.last_decay, ema.get_decay())
    assert mine.counter == ema.update_freq_counter
    theirs = flat(ema.fp32_params)
    assert theirs.dtype == torch.float32
    assert torch.equal(mine.e32.view(torch.int32), theirs.view(torch.int32)), updates
    assert torch.equal(mine.e16.view(torch.int16), flat(ema.get_model().state_dict()).view(torch.int16)), updates
assert stepped == 3
print("EMA-OK")
'''


def _fairseq_source():
    """"installed" | "reference" (the vendored copy of a reference checkout, through oracle/_refshim.py) | None"""
    if importlib.util.find_spec("fairseq") is not None:
        return "installed"
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import _refshim
    finally:
        sys.path.pop(0)
    if _refshim.reference_available() and os.path.isdir(os.path.join(_refshim.REFERENCE_ROOT, "custom_fairseq", "fairseq")):
        return "reference"
    return None


def test_schedule_and_rule_reproduce_fairseqs_ema_class():
    """a bf16 nn.Linear under fairseq's EMA(ema_fp32, decay 0.99, start 2, freq 2), six updates with changing weights: the
    schedule, the counter and the rule of this module give its fp32_params and its 16-bit model bit for bit"""
    src = _fairseq_source()
    if src is None:
        pytest.skip("needs fairseq: not installed, and no reference checkout with its vendored copy (IFSEG_REFERENCE_ROOT)")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, "1" if src == "reference" else "0"], capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0 and "EMA-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def _student(n=1027, seed=5):
    e, p = arenas(n, seed)
    return e.clone(), e.to(torch.bfloat16)


def test_arena_ema_cpu_schedule_swap_and_state_dict():
    from ifseg_amd.ema import ArenaEMA, ema_reference
    p32, p16 = _student()
    ema = ArenaEMA(p32, p16, decay=0.5, start_update=2, update_freq=2, device="cpu")
    assert ema.fresh and torch.equal(ema.e32, p32) and torch.equal(ema.e16.view(torch.int16), p16.view(torch.int16))
    want32, steps = ema.e32.clone(), []
    g = torch.Generator().manual_seed(6)
    for updates in range(1, 7):
        p32.add_(torch.randn(p32.shape, generator=g) * 0.05)
        p16.copy_(p32)
        steps.append(ema.update(updates) is not None)
        if steps[-1]:
            want32, want16 = ema_reference(want32, p16, 0.0 if updates < 2 else 0.5)
            assert torch.equal(ema.e32.view(torch.int32), want32.view(torch.int32))
            assert torch.equal(ema.e16.view(torch.int16), want16.view(torch.int16))
    assert steps == [False, True] * 3 and not ema.fresh
    # the swap round trip
    snap = [t.clone() for t in (p32, p16, ema.e32, ema.e16)]
    ema.swap()
    assert ema.swapped
    for got, want in zip((p32, p16, ema.e32, ema.e16), (snap[2], snap[3], snap[0], snap[1])):
        assert torch.equal(got.view(torch.int32 if got.dtype == torch.float32 else torch.int16),
                           want.view(torch.int32 if want.dtype == torch.float32 else torch.int16))
    with pytest.raises(RuntimeError, match="swapped"):
        ema.state_dict()
    ema.swap()
    assert not ema.swapped and all(torch.equal(a, b) for a, b in zip((p32, p16, ema.e32, ema.e16), snap))
    # state_dict -> load_state_dict
    sd = ema.state_dict()
    other = ArenaEMA(p32.clone(), p16.clone(), decay=0.5, start_update=2, update_freq=2)
    other.counter = 1
    other.load_state_dict(sd)
    assert torch.equal(other.e32, ema.e32) and torch.equal(other.e16.view(torch.int16), ema.e16.view(torch.int16))
    assert other.counter == ema.counter and other.last_decay == ema.last_decay and not other.fresh
    assert sd["e32"].data_ptr() != ema.e32.data_ptr()


def test_arenas_are_refused_by_name():
    from ifseg_amd import hip
    from ifseg_amd.ema import ArenaEMA
    p32, p16 = _student(64)
    e32, e16 = p32.clone(), p16.clone()
    with pytest.raises(ValueError, match="p32 must be a torch.float32"):
        ArenaEMA(p32.double(), p16)
    with pytest.raises(ValueError, match="p16 must be a torch.bfloat16"):
        ArenaEMA(p32, p16.float())
    with pytest.raises(ValueError, match="p16 has 63 elements"):
        ArenaEMA(p32, p16[:63])
    with pytest.raises(ValueError, match="device"):
        ArenaEMA(p32, p16, device="cuda:0")
    both = torch.zeros(96)
    with pytest.raises(ValueError, match="p32 and p16 overlap"):
        ArenaEMA(both[:64], both[48:80].view(torch.bfloat16))
    # the bindings refuse before anything reaches the library
    with pytest.raises(ValueError, match="p32 and e32 overlap"):
        hip.ema_swap(both[:64], p16, both[32:96], e16)
    half = torch.zeros(96, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="p16 and e16 overlap"):
        hip.ema_swap(p32, half[:64], e32, half[32:])
    with pytest.raises(ValueError, match="e32 must be a torch.float32"):
        hip.ema_swap(p32, p16, e16, e16)
    with pytest.raises(ValueError, match="e16 has 32 elements"):
        hip.ema_swap(p32, p16, e32, e16[:32])
    with pytest.raises(ValueError, match="e16 must be a torch.bfloat16"):
        hip.adam_ema_step(p32, p16, p32, p32, p16, e32, e32, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, 0.5, 0.5)


def test_surface():
    from ifseg_amd import hip
    from ifseg_amd.trainer import Trainer
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    names = set(re.findall(r"\bint\s+(ifseg_\w+)\s*\(", hdr))
    assert {"ifseg_adam_ema_step", "ifseg_ema_swap", "ifseg_adam_step"} <= names
    assert int(re.search(r"#define IFSEG_ABI_VERSION (\d+)", hdr).group(1)) == 21 == hip.ABI_VERSION
    assert callable(hip.adam_ema_step) and callable(hip.ema_swap)
    if os.path.exists(hip.LIB_PATH):
        lib = hip.lib()
        assert hasattr(lib, "ifseg_adam_ema_step") and hasattr(lib, "ifseg_ema_swap")
    par = inspect.signature(Trainer).parameters
    assert [(k, par[k].default) for k in ("store_ema", "ema_decay", "ema_start_update", "ema_update_freq")] == \
        [("store_ema", False), ("ema_decay", 0.9999), ("ema_start_update", 0), ("ema_update_freq", 1)]
    assert callable(Trainer.ema_weights) and callable(Trainer.ema_state_dict) and callable(Trainer.load_ema_state_dict)
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    assert inspect.signature(SegmentationTask.self_train_sample).parameters["trainer"].default is None
