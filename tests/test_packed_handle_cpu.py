"""``_native.PackedHandle`` / ``OwnedHandle`` / ``compute_mode`` and ``convert.read_state_dict`` on the host: the owner is driven with
recording fakes in place of a native family, so no kernel runs and the device named in a token is never touched."""
import copy
import ctypes as C
import gc
import pickle

import pytest
import torch

from streamformer_amd import _native as nat
from streamformer_amd.convert import read_state_dict, write_state_dict

CUDA0, CUDA1 = torch.device("cuda", 0), torch.device("cuda", 1)


class Family:
    """A fake native family: every call is appended to ``log``; handles are the integers 1, 2, ..."""

    def __init__(self):
        self.log, self.made = [], 0

    def create(self, device_index, key=None):
        self.made += 1
        self.log.append(("create", device_index, key, self.made))
        return self.made

    def load_tensor(self, h, name, ptr, code, shape, ndim):
        self.log.append(("load", h, name.decode(), code, tuple(shape[:ndim])))
        return nat.SF_OK

    def finalize(self, h):
        self.log.append(("finalize", h))

    def destroy(self, h):
        self.log.append(("destroy", h))

    def on_release(self):
        self.log.append(("on_release",))

    def owner(self, **kw):
        return nat.PackedHandle(self.create, self.load_tensor, self.finalize, self.destroy, "thing", **kw)

    def take(self):
        log, self.log = self.log, []
        return log


@pytest.fixture(autouse=True)
def no_device_guard(monkeypatch):
    class Guard:
        def __init__(self, device):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(torch.cuda, "device", Guard)


def _items():
    return [("b", torch.zeros(3)), ("a", torch.ones(2, 2))]


def _packed(h, dev=0, key=None):
    return [("create", dev, key, h), ("load", h, "b", nat.SF_F32, (3,)), ("load", h, "a", nat.SF_F32, (2, 2)), ("finalize", h)]


def test_same_token_makes_no_native_call():
    fam = Family()
    own = fam.owner()
    items = _items()
    tok = nat.weights_token(CUDA0, [t for _, t in items])
    assert own.get(CUDA0, tok, items) == 1
    assert fam.take() == _packed(1)                                  # create, loads in item order, finalize
    listed = []
    assert own.get(CUDA0, nat.weights_token(CUDA0, [t for _, t in items]), lambda: listed.append(1) or items) == 1
    assert fam.take() == [] and listed == [] and own.token == tok    # nothing stale: nothing listed, nothing called


@pytest.mark.parametrize("change", ["version", "data_ptr", "device"])
def test_changed_token_repacks(change):
    fam = Family()
    own = fam.owner(on_release=fam.on_release)
    items = _items()
    own.get(CUDA0, nat.weights_token(CUDA0, [t for _, t in items]), items)
    own.workspace(1000, torch.device("cpu"))
    fam.take()
    dev = CUDA0
    if change == "version":
        items[0][1].add_(1)
    elif change == "data_ptr":
        items[1] = ("a", torch.ones(2, 2))
    else:
        dev = CUDA1
    tok = nat.weights_token(dev, [t for _, t in items])
    assert tok != own.token
    assert own.get(dev, tok, lambda: items) == 2
    assert fam.take() == [("on_release",), ("destroy", 1)] + _packed(2, dev.index)
    assert own.workspaces == {} and own.token == tok                        # the workspace went with the old packing


def test_keyed_handles_share_one_token():
    fam = Family()
    own = fam.owner(on_release=fam.on_release)
    items = _items()
    tok = nat.weights_token(CUDA0, [t for _, t in items])
    assert [own.get(CUDA0, tok, items, key) for key in ("x", "y", "x")] == [1, 2, 1]
    assert fam.take() == _packed(1, key="x") + _packed(2, key="y") and sorted(own.handles) == ["x", "y"]
    items[0][1].mul_(2)
    assert own.get(CUDA0, nat.weights_token(CUDA0, [t for _, t in items]), items, "y") == 3
    assert fam.take() == [("on_release",), ("destroy", 1), ("destroy", 2)] + _packed(3, key="y")
    assert list(own.handles) == ["y"]


def test_refuses_a_module_that_is_not_on_the_gpu():
    fam = Family()
    with pytest.raises(RuntimeError, match=r"the thing runs on the MI355X: move the module with \.to\('cuda'\) \(there is no CPU fallback\)"):
        fam.owner().get(torch.device("cpu"), 1, [])
    with pytest.raises(RuntimeError, match="^its own words$"):
        fam.owner(refusal="its own words").get(torch.device("cpu"), 1, [])
    assert fam.log == []


def test_failed_pack_keeps_nothing():
    fam = Family()

    def finalize(h):
        raise nat.NativeError(nat.SF_ERR_STATE, "missing 1 weights: a")

    own = nat.PackedHandle(fam.create, fam.load_tensor, finalize, fam.destroy, "thing")
    with pytest.raises(nat.NativeError, match="missing 1 weights"):
        own.get(CUDA0, 7, [])
    assert fam.take() == [("create", 0, None, 1), ("destroy", 1)] and own.handles == {}


def test_release_destroys_once():
    fam = Family()
    own = fam.owner()
    own.get(CUDA0, 1, [])
    fam.take()
    own.release()
    own.release()
    assert fam.take() == [("destroy", 1)] and own.handles == {} and own.token is None
    own.__del__()
    del own
    assert fam.take() == []
    own = fam.owner()
    own.get(CUDA0, 1, [])
    fam.take()
    del own                                                          # no cycle through the bound methods: freed with its last reference
    assert fam.take() == [("destroy", 2)]


def test_bound_methods_are_held_weakly():
    class Module:
        def __init__(self, fam):
            self.native = nat.PackedHandle(self.create, fam.load_tensor, fam.finalize, fam.destroy, "thing", on_release=self.hook)
            self.create_ = fam.create

        def create(self, device_index):
            return self.create_(device_index)

        def hook(self):
            raise AssertionError("the module is gone")

    fam = Family()
    gc.disable()
    try:
        m = Module(fam)
        m.native.get(CUDA0, 1, [])
        cache = nat.OwnedHandle(fam.destroy, "cache")                # made against the packed handle, outlives the module
        cache.value = 77
        m.native.dependents.add(cache)
        fam.take()
        del m                                                        # the cycle collector is off: reference counting alone frees both
        assert fam.take() == [("destroy", 77), ("destroy", 1)] and not cache          # the hook is skipped, the dependents are not
    finally:
        gc.enable()


def test_workspace_grows_only():
    fam = Family()
    own = fam.owner()
    own.get(CUDA0, 1, [])
    cpu, meta = torch.device("cpu"), torch.device("meta")
    a = own.workspace(1000, cpu)
    assert a.dtype == torch.uint8 and a.numel() == 1000
    assert own.workspace(10, cpu) is a and own.workspace(1000, cpu) is a          # never shrinks
    b = own.workspace(1001, cpu)
    assert b is not a and b.numel() == 1001 and own.workspace(1000, cpu) is b
    c = own.workspace(10, meta)                                                   # another device: a new buffer there
    assert c.device == meta and c.numel() == 256
    k1, k2 = own.workspace(300, cpu, key=(1, 2)), own.workspace(400, cpu, key=(3, 4))
    assert own.workspace(300, cpu, key=(1, 2)) is k1 and own.workspace(400, cpu, key=(3, 4)) is k2
    own.workspaces.clear()                                                        # a module that holds one shape at a time
    k3 = own.workspace(500, cpu, key=(5, 6))
    assert list(own.workspaces.values()) == [k3]
    assert own.get(CUDA0, 1, []) == 1 and list(own.workspaces.values()) == [k3]
    assert own.get(CUDA0, 2, []) == 2 and own.workspaces == {}                           # a repack drops it


def test_copies_are_empty_owners():
    fam = Family()
    own = fam.owner(on_release=fam.on_release)
    own.get(CUDA0, 1, [], "x")
    own.get(CUDA0, 1, [], "y")
    own.workspace(300, torch.device("cpu"))
    fam.take()
    for twin, other in (copy.deepcopy((fam, own)), pickle.loads(pickle.dumps((fam, own)))):      # (the family is held as a module holds itself)
        assert isinstance(other, nat.PackedHandle) and other is not own and twin is not fam
        assert other.handles == {} and other.token is None and other.workspaces == {} and len(other.dependents) == 0
        assert other._family[0]().__self__ is twin                   # the callables went along: the copy serves the copied family
        assert other.get(CUDA0, 5, []) == twin.made and twin.log[-2:] == [("create", 0, None, twin.made), ("finalize", twin.made)]
        del other, twin
    assert fam.take() == []                                          # the copies never touched the original's handles
    del own
    assert fam.take() == [("on_release",), ("destroy", 1), ("destroy", 2)]


def test_library_entry_points_are_kept_by_name():
    own = nat.PackedHandle(None, nat.lib.sf_text_load_tensor, None, nat.lib.sf_text_destroy, "thing")
    for other in (own, copy.deepcopy(own), pickle.loads(pickle.dumps(own))):      # ctypes function pointers do neither
        assert other._family[1] == "sf_text_load_tensor" and nat._strong(other._family[3]).__name__ == "sf_text_destroy"


def test_owned_handle():
    log = []
    h = nat.OwnedHandle(log.append, "probe")
    assert not h and isinstance(h, C.c_void_p)
    C.cast(C.byref(h), C.POINTER(C.c_void_p))[0] = 0x1234            # what a *_create does through byref
    assert h and h.value == 0x1234
    for copier in (copy.copy, copy.deepcopy, pickle.dumps):
        with pytest.raises(TypeError, match="a probe is device memory of one native handle and cannot be copied or pickled"):
            copier(h)
    h.release()
    h.release()
    assert log == [0x1234] and not h
    del h
    g = nat.OwnedHandle(log.append, "probe")
    g.value = 7
    del g
    assert log == [0x1234, 7]


class EntryPoint:
    """A fake library entry point: records its arguments, answers ``code``; ``size`` is what a sizer writes through its last argument."""

    def __init__(self, code=nat.SF_OK, size=None):
        self.code, self.size, self.calls = code, size, []

    def __call__(self, *args):
        self.calls.append(args)
        if self.size is not None:
            args[-1]._obj.value = self.size
        return self.code


@pytest.fixture
def guard_log(monkeypatch):
    """``torch.cuda.device`` records ("enter" | "exit", device); cuda:0 is the current device; the stream of a device is 0x5000 + its
    index."""
    log = []

    class Guard:
        def __init__(self, device):
            self.device = device

        def __enter__(self):
            log.append(("enter", self.device))

        def __exit__(self, *exc):
            log.append(("exit", self.device))
            return False

    monkeypatch.setattr(torch.cuda, "device", Guard)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(nat, "current_stream_handle", lambda device: 0x5000 + (device.index or 0))
    return log


def test_launch_passes_arguments_through_with_the_stream_last(guard_log):
    fn, t = EntryPoint(), torch.zeros(3)
    assert nat.launch(CUDA1, fn, 7, None, 2.5, t) is None
    assert len(fn.calls) == 1 and len(fn.calls[0]) == 5
    assert fn.calls[0][:3] == (7, None, 2.5) and fn.calls[0][3] is t and fn.calls[0][4] == 0x5001
    assert guard_log == [("enter", CUDA1), ("exit", CUDA1)]


def test_launch_enters_no_guard_when_the_device_is_current(guard_log):
    fn = EntryPoint()
    nat.launch(CUDA0, fn)
    nat.launch(torch.device("cuda"), fn, 3)                           # no index: the current device
    assert fn.calls == [(0x5000,), (3, 0x5000)] and guard_log == []


def test_launch_workspace_tail(guard_log):
    fn, ws = EntryPoint(), torch.empty(300, dtype=torch.uint8)
    nat.launch(CUDA0, fn, 1, 2, workspace=ws)
    nat.launch(CUDA0, fn, 1, 2, workspace=None)
    assert fn.calls == [(1, 2, ws.data_ptr(), 300, 0x5000), (1, 2, 0, 0, 0x5000)]


def test_launch_raises_the_code_and_leaves_the_guard(guard_log):
    with pytest.raises(nat.NativeError) as e:
        nat.launch(CUDA1, EntryPoint(nat.SF_ERR_WORKSPACE), 1, workspace=None)
    assert e.value.code == nat.SF_ERR_WORKSPACE
    assert guard_log == [("enter", CUDA1), ("exit", CUDA1)]

    def broken(*args):
        raise KeyError("inside the call")

    with pytest.raises(KeyError):
        nat.launch(CUDA1, broken)
    assert guard_log[2:] == [("enter", CUDA1), ("exit", CUDA1)]


def test_sized():
    fn = EntryPoint(size=12345)
    assert nat.sized(fn, 4, 5) == 12345
    assert len(fn.calls[0]) == 3 and fn.calls[0][:2] == (4, 5) and isinstance(fn.calls[0][2]._obj, C.c_size_t)
    with pytest.raises(nat.NativeError) as e:
        nat.sized(EntryPoint(nat.SF_ERR_INVALID, size=1), 4)
    assert e.value.code == nat.SF_ERR_INVALID


def test_scratch_has_the_workspace_floor():
    cpu = torch.device("cpu")
    s = nat.scratch(0, cpu)
    assert s.dtype == torch.uint8 and s.device == cpu and s.numel() == 256 == nat.WORKSPACE_FLOOR
    assert nat.scratch(255, cpu).numel() == 256 and nat.scratch(257, cpu).numel() == 257
    assert nat.PackedHandle().workspace(0, cpu).numel() == s.numel()            # the two allocators agree


def test_ctypes_arrays():
    a, b = torch.zeros(2), torch.ones(5)
    p = nat.ptr_array([a, None, b])
    assert isinstance(p, C.Array) and p._type_ is C.c_void_p and list(p) == [a.data_ptr(), None, b.data_ptr()]
    i = nat.i32_array([3, torch.Size([9])[0], -1])
    assert i._type_ is C.c_int32 and list(i) == [3, 9, -1]
    assert len(nat.ptr_array([])) == 1 and len(nat.i32_array([])) == 1          # never a zero-length array: its address is passed


PARENT_TABLES = {       # what each module's own table took before there was one
    "text": {"bf16": 0, "fp32": 1, "bf16x3": 1},
    "connector": {"bf16": 0, "fp32": 1, "bf16x3": 1},
    "oad": {"bf16": 0, torch.bfloat16: 0, "fp32": 1, "bf16x3": 1, torch.float32: 1},
    "msda": {"bf16": 0, torch.bfloat16: 0, "fp32": 1, "bf16x3": 1, torch.float32: 1},
    "modeling": {"bf16": 0, "bfloat16": 0, torch.bfloat16: 0, "bf16x3": 1, "fp32": 1, "float32": 1, torch.float32: 1},
}


def test_compute_mode():
    assert (nat.SF_COMPUTE_BF16, nat.SF_COMPUTE_BF16X3) == (0, 1)
    for table in PARENT_TABLES.values():
        for value, code in table.items():
            assert nat.compute_mode(value) == code, value
    for bad in ("fp16", None, torch.float16, 0):
        with pytest.raises(ValueError) as e:
            nat.compute_mode(bad)
        assert str(e.value) == f"compute_dtype must be one of 'bf16' (throughput) or 'fp32'/'bf16x3' (accurate), got {bad!r}"


def test_read_state_dict(tmp_path):
    d = str(tmp_path)
    names = ("a.bin", "b.safetensors", "c.safetensors")
    with pytest.raises(OSError) as e:
        read_state_dict(d, names)
    assert str(e.value) == f"no a.bin / b.safetensors / c.safetensors under {d!r}"
    with pytest.raises(OSError) as e:
        read_state_dict(d, ("model.safetensors", "pytorch_model.bin", "model.bin"))
    assert str(e.value) == f"no model.safetensors / pytorch_model.bin under {d!r}"
    x = torch.arange(6.0).reshape(2, 3).t()                          # not contiguous: the writer makes it so
    write_state_dict(d, {"w": x, "c": torch.ones(1) * 3}, "c.safetensors", True)
    got = read_state_dict(d, names)
    assert set(got) == {"w", "c"} and torch.equal(got["w"], x) and float(got["c"]) == 3.0
    write_state_dict(d, {"w": x + 1}, "b.safetensors", True)
    assert torch.equal(read_state_dict(d, names)["w"], x + 1)        # the order of `names` decides, not the directory's
    write_state_dict(d, {"w": x + 2}, "a.bin", False)
    assert torch.equal(read_state_dict(d, names)["w"], x + 2)
    assert torch.equal(torch.load(str(tmp_path / "a.bin"), weights_only=True)["w"], x + 2)        # the .bin branch is torch.save
    assert torch.equal(read_state_dict(d, names[::-1])["w"], x)
