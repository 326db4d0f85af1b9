"""CPU: the whole dispatcher surface of ifseg_amd/ops.py, pinned (tests/_ops_cases.py is the record): the set of `ifseg::*` ops,
every schema, the fake outputs of one good call per op, and the complete message of every refusal probe -- under FakeTensorMode
with `hip.lib` patched to raise, so nothing is launched and the library is not loaded.  And the stream scope every op body runs
in: what it pins and that it restores it."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import _ops_cases as C
from ifseg_amd import hip, ops  # noqa: F401  (registers torch.ops.ifseg)


def _registered():
    return {s.name.split("::")[1] for s in torch._C._jit_get_all_schemas() if s.name.startswith("ifseg::")}


@pytest.fixture
def no_lib(monkeypatch):
    def refuse():
        raise AssertionError("hip.lib() touched under FakeTensorMode")
    monkeypatch.setattr(hip, "lib", refuse)


def _call(op, changes=None):
    args = dict(C.GOOD[op][0])
    args.update(changes or {})
    return getattr(torch.ops.ifseg, op)(**{k: C.real(v) for k, v in args.items()})


def test_the_set_of_ops_is_the_recorded_one():
    assert _registered() == set(C.SCHEMAS)
    assert set(C.GOOD) == set(C.SCHEMAS)


@pytest.mark.parametrize("op", sorted(C.SCHEMAS))
def test_schema(op):
    assert str(getattr(torch.ops.ifseg, op).default._schema) == C.SCHEMAS[op]


@pytest.mark.parametrize("op", sorted(C.GOOD))
def test_good_call_gives_the_recorded_shapes_and_dtypes(op, no_lib):
    with FakeTensorMode():
        out = _call(op)
        out = (out,) if torch.is_tensor(out) else tuple(out)
        assert [(tuple(o.shape), o.dtype) for o in out] == C.GOOD[op][1]
        assert all(o.device.type == "cuda" for o in out)


def _own_words(exc):
    """the message without what the dispatcher puts around it: the refusal starts at the op's name"""
    text = str(exc)
    return text[text.index("ifseg::"):] if "ifseg::" in text else text


@pytest.mark.parametrize("k", range(len(C.PROBES)), ids=["%s-%d" % (p[0], k) for k, p in enumerate(C.PROBES)])
def test_refusal_message(k, no_lib):
    op, changes, message = C.PROBES[k]
    with FakeTensorMode():
        with pytest.raises((ValueError, RuntimeError)) as e:
            _call(op, changes)
    assert _own_words(e.value) == message


# ------------------------------------------------------------------------------------------------------- the stream scope
class _Stream:
    def __init__(self, handle):
        self.cuda_stream = handle


@pytest.fixture
def streams(monkeypatch):
    """torch.cuda.current_stream -> a stub whose handle is the next of 101, 102, ...; hip's pin starts at a marker"""
    seen = []

    def current_stream(device=None):
        seen.append(device)
        return _Stream(100 + len(seen))
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    monkeypatch.setattr(hip, "_stream_handle", 7)
    return seen


def test_scope_pins_the_current_stream_and_restores_the_previous(streams):
    x = torch.empty(1)
    with ops._on_stream(x):
        assert hip._stream_handle == 101
    assert hip._stream_handle == 7 and streams == [x.device]
    with ops._on_stream(torch.device("cuda", 0)):                  # a device instead of a tensor (strong_draw)
        assert hip._stream_handle == 102
    assert hip._stream_handle == 7 and streams[1] == torch.device("cuda", 0)


def test_scope_restores_after_an_exception(streams):
    with pytest.raises(KeyError):
        with ops._on_stream(torch.empty(1)):
            assert hip._stream_handle == 101
            raise KeyError("inside")
    assert hip._stream_handle == 7


def test_scopes_nest_and_restore_in_order(streams):
    x = torch.empty(1)
    with ops._on_stream(x):
        with ops._on_stream(x):
            assert hip._stream_handle == 102
            with pytest.raises(KeyError):
                with ops._on_stream(x):
                    assert hip._stream_handle == 103
                    raise KeyError("innermost")
            assert hip._stream_handle == 102
        assert hip._stream_handle == 101
    assert hip._stream_handle == 7
