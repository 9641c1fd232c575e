"""The shared host plumbing of cmgan_amd.engine on the CPU (no GPU, no library): the one tensor-argument rule
(tensor_arg), the pointer conversion of a native call (native_call) and the grow-only workspaces (Engine._grow)."""
import ctypes
import types
import weakref

import pytest
import torch

from cmgan_amd import engine as E
from cmgan_amd.engine import Engine, native_call, tensor_arg

CPU, META = torch.device("cpu"), torch.device("meta")
FLAT4 = ("[4]", lambda t: tuple(t.shape) == (4,))


def test_a_good_argument_is_returned_as_it_is():
    t = torch.zeros(4)
    assert tensor_arg(t, "x", torch.float32, CPU, *FLAT4) is t
    assert tensor_arg(t, "x", torch.float32, CPU) is t                              # no shape rule
    m = torch.zeros(4, dtype=torch.int32, device=META)
    assert tensor_arg(m, "x", torch.int32, META, *FLAT4) is m


@pytest.mark.parametrize("arg,kind,text", [
    ([0.0] * 4, TypeError, "x: expected a torch.Tensor, got list"),
    (torch.zeros(4, dtype=torch.float64), TypeError, "x: expected float32, got float64"),
    (torch.zeros(4, device=META), RuntimeError, "x: tensor is on meta but this Engine is bound to cpu"),
    (torch.zeros(5), ValueError, r"x: expected \[4\], got \(5,\)"),
    (torch.zeros(8)[::2], ValueError, "x: must be contiguous"),
])
def test_every_rule_has_its_exception_type_and_names_the_argument(arg, kind, text):
    with pytest.raises(kind, match=text) as e:
        tensor_arg(arg, "x", torch.float32, CPU, *FLAT4)
    assert type(e.value) is kind
    # error=: the same message under the one type the stream arguments have always raised
    with pytest.raises(ValueError, match=text) as e:
        tensor_arg(arg, "x", torch.float32, CPU, *FLAT4, error=ValueError)
    assert type(e.value) is ValueError


def test_the_rules_are_checked_in_order_type_dtype_device_shape_contiguity():
    wrong = torch.zeros(5, 2, dtype=torch.float64, device=META)[:, 0]               # everything is wrong with it
    with pytest.raises(TypeError, match="expected float32"):
        tensor_arg(wrong, "x", torch.float32, CPU, *FLAT4)
    with pytest.raises(RuntimeError, match="is on meta"):
        tensor_arg(wrong, "x", torch.float64, CPU, *FLAT4)
    with pytest.raises(ValueError, match=r"expected \[4\]"):
        tensor_arg(wrong, "x", torch.float64, META, *FLAT4)
    with pytest.raises(ValueError, match="must be contiguous"):
        tensor_arg(wrong, "x", torch.float64, META, "[5]", lambda t: t.numel() == 5)


def test_contiguity_is_the_callers_when_it_says_so():
    t = torch.zeros(8)[::2]
    assert tensor_arg(t, "x", torch.float32, CPU, *FLAT4, contiguous=False) is t
    with pytest.raises(ValueError, match=r"x: expected \[4\]"):                     # (the other rules still hold)
        tensor_arg(torch.zeros(10)[::2], "x", torch.float32, CPU, *FLAT4, contiguous=False)


def test_the_device_rule_compares_devices_not_device_types():
    t = torch.zeros(4, device=META)
    with pytest.raises(RuntimeError, match="x: tensor is on meta but this Engine is bound to cuda:0"):
        tensor_arg(t, "x", torch.float32, torch.device("cuda:0"), *FLAT4)
    with pytest.raises(RuntimeError, match="x: tensor is on cpu but this Engine is bound to meta"):
        tensor_arg(torch.zeros(4), "x", torch.float32, META, *FLAT4)


# ---- native_call: (handle, *converted arguments), checked ------------------------------------------------------------
class _Params(ctypes.Structure):
    _fields_ = [("a", ctypes.c_int), ("b", ctypes.c_void_p)]


class _RecordingLib:
    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.rc
        return fn


def test_native_call_converts_tensors_none_structs_and_passes_the_rest():
    stub = types.SimpleNamespace(lib=_RecordingLib(), _h=ctypes.c_void_p(7))
    t, p = torch.arange(6.0), _Params(3, 99)
    native_call(stub, "cmgan_something", t, None, p, 5, 0.25, t[2:])
    (name, args), = stub.lib.calls
    assert name == "cmgan_something" and len(args) == 7
    assert args[0] is stub._h                                                       # the handle goes first
    assert args[1] == t.data_ptr() and args[2] is None and args[4] == 5 and args[5] == 0.25
    assert args[6] == t.data_ptr() + 2 * 4                                          # a view: ITS first element
    assert type(args[3]) is type(ctypes.byref(p)) and args[3]._obj is p             # by reference: the caller's struct itself


def test_native_call_checks_the_return_code(monkeypatch):
    seen = []
    monkeypatch.setattr(E, "check", lambda handle, rc: seen.append((handle, rc)))
    stub = types.SimpleNamespace(lib=_RecordingLib(rc=-3), _h=ctypes.c_void_p(7))
    native_call(stub, "cmgan_other")
    assert seen == [(stub._h, -3)] and stub.lib.calls == [("cmgan_other", (stub._h,))]


# ---- Engine._grow on the CPU: the allocation device is the stub's ----------------------------------------------------
def _grower():
    evicted = []
    stub = types.SimpleNamespace(_wss={}, device=CPU, evicted=evicted,
                                 _EVICT={"main": lambda self: evicted.append("main"),
                                         "branched": lambda self: evicted.append("branched")})
    return stub, lambda slot, need, bad=None: Engine._grow(stub, slot, need, bad)


def test_grow_allocates_once_and_only_grows():
    stub, grow = _grower()
    a = grow("mix", 100)
    assert a.dtype == torch.uint8 and a.device == CPU and a.numel() == 100 and stub._wss == {"mix": a}
    assert grow("mix", 100) is a and grow("mix", 1) is a                            # holds it: the same tensor
    b = grow("mix", 101)
    assert b is not a and b.numel() == 101 and grow("mix", 100) is b                # grew, and never shrinks
    key = ("resample", 48000, 16000)                                                # any hashable names a slot
    r = grow(key, 8)
    assert grow(key, 8) is r and stub._wss[key] is r and stub._wss["mix"] is b
    assert stub.evicted == []                                                       # no graph points into these slots


def test_grow_drops_the_old_allocation_before_it_allocates(monkeypatch):
    stub, grow = _grower()
    old = weakref.ref(grow("rir", 64))
    alive_at_allocation = []
    real_empty = torch.empty

    def empty(*a, **k):
        alive_at_allocation.append(old() is not None)
        return real_empty(*a, **k)
    monkeypatch.setattr(E.torch, "empty", empty)
    assert grow("rir", 64).numel() == 64 and alive_at_allocation == []              # held: no allocation at all
    assert grow("rir", 65).numel() == 65
    assert alive_at_allocation == [False] and old() is None                         # the peak is not old + new


def test_grow_refuses_zero_bytes_with_the_callers_message():
    stub, grow = _grower()
    with pytest.raises(ValueError, match=r"^bad batch/frames \(0, 3\)$"):
        grow("main", 0, "bad batch/frames (0, 3)")
    assert stub._wss == {} and stub.evicted == []                                   # refused before anything happened
    assert grow("conformer", 0).numel() == 0                                        # no message: an empty workspace


def test_eviction_fires_when_its_slot_grows_and_not_otherwise():
    stub, grow = _grower()
    grow("main", 10)
    assert stub.evicted == ["main"]                                                 # the first allocation counts as growth
    grow("main", 10), grow("main", 4), grow("metrics", 50), grow("metrics", 60)
    assert stub.evicted == ["main"]
    grow("branched", 20)
    assert stub.evicted == ["main", "branched"]
    grow("main", 11)
    assert stub.evicted == ["main", "branched", "main"]
    grow("branched", 20)
    assert stub.evicted == ["main", "branched", "main"]


def test_the_engines_eviction_rules_are_the_two_that_captured_graphs_need():
    """Main workspace: the one-branch graphs, every row graph, every stream slot's step and stage graphs.  Branched
    workspace: the multi-branch graphs.  Nothing else is touched."""
    assert set(Engine._EVICT) == {"main", "branched"}
    slot = types.SimpleNamespace(graphs={"s": 1}, stage_graphs={"t": 2})
    mk = lambda: types.SimpleNamespace(_graphs={((2, 4000), 1, 0): "one", ((2, 4000), 2, 0): "two"},
                                       _row_graphs={"rows": 3}, _stream_slots={"k": slot})
    e = mk()
    Engine._EVICT["main"](e)
    assert e._graphs == {((2, 4000), 2, 0): "two"} and not e._row_graphs
    assert not slot.graphs and not slot.stage_graphs and list(e._stream_slots) == ["k"]
    slot.graphs["s"] = 1
    e = mk()
    Engine._EVICT["branched"](e)
    assert e._graphs == {((2, 4000), 1, 0): "one"} and e._row_graphs == {"rows": 3} and slot.graphs == {"s": 1}
