"""Shared test helpers: seeded inputs identical to oracle/make_golden.py, small configs, the precision-floor rule, guard buffers, metrics."""
import numpy as np
import torch

from streamformer_amd.configuration import StreamformerConfig


def small_cfg(**kw):
    base = dict(image_size=48, patch_size=16, num_frames=16, hidden_size=128, num_hidden_layers=2,
                num_attention_heads=2, intermediate_size=256, enable_causal_temporal=True)
    base.update(kw)
    return StreamformerConfig(**base)


def frames(seed, shape, clamp=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    return x.clamp_(-1, 1) if clamp else x


def maxabs(a, b):
    a = torch.as_tensor(np.asarray(a)) if not torch.is_tensor(a) else a
    b = torch.as_tensor(np.asarray(b)) if not torch.is_tensor(b) else b
    return float((a.double().cpu() - b.double().cpu()).abs().max())


# ---------------------------------------------------------------------------------------------------
# precision floors: a bound is MARGIN times the error, against fp64, of the same operator sequence in torch at the operand precision of
# the code under test, and never less than one fp32 rounding of the result
# ---------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24
MARGIN = 4.0


def fp32_floor(got32, want):
    """Precision floor of a computation: what its torch restatement ``got32`` loses against fp64, at least one fp32 rounding of ``want``."""
    return max(maxabs(got32, want), EPS32 * float(want.abs().max()))


def check_against_floor(what, got, floor32, want, margin=MARGIN):
    bound = margin * fp32_floor(floor32, want)
    err = maxabs(got, want)
    print(f"  {what}: error {err:.3e}, bound {bound:.3e} ({err / bound:.3f})")
    assert err <= bound, (what, err, bound)


# ---------------------------------------------------------------------------------------------------
# guard buffers: an out-of-bounds or a missing store of a kernel shows as a NaN in the wrong place
# ---------------------------------------------------------------------------------------------------
def guarded(dev, *shape):
    """A NaN-filled buffer with one guard row behind the tensor: (whole buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), float("nan"), device=dev)
    return buf, buf[:n].view(*shape)


def read_guarded(buf, view):
    """The view's CPU copy, after asserting that the guard row is untouched and that every element of the view was written."""
    host = buf.cpu()
    assert torch.isnan(host[view.numel():]).all(), "the guard row was written"
    assert not torch.isnan(host[:view.numel()]).any(), "output elements left unwritten"
    return host[:view.numel()].view(view.shape)


def guarded_ints(dev, n, fill=0x5a5a5a5a):
    """An int32 buffer of n elements with 64 guard words behind it."""
    return torch.full((n + 64,), fill, dtype=torch.int32, device=dev)


def read_guarded_ints(buf, n, fill=0x5a5a5a5a):
    host = buf.cpu()
    assert (host[n:] == fill).all(), "the guard words were written"
    return host[:n]


# ---------------------------------------------------------------------------------------------------
# the native library as the tests reach it
# ---------------------------------------------------------------------------------------------------
def native():
    """streamformer_amd._native, imported on first use: collecting a test file must not need the built library."""
    import streamformer_amd._native as nat
    return nat


def stream():
    return native().current_stream_handle(gpu_device())


class NoLaunch:
    """Stands in for the module's view of streamformer_amd._native: size and capacity queries pass, every other entry point of the
    library is recorded in ``calls`` and refused, so a refusal that came after a launch cannot pass for one that came before."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    @property
    def lib(self):
        outer = self

        class Lib:
            def __getattr__(self, name):
                if name.endswith(("_workspace_bytes", "_capacity")) or name == "sf_last_error":
                    return getattr(outer._real.lib, name)
                outer.calls.append(name)
                raise AssertionError(f"{name} was reached")
        return Lib()


# ---------------------------------------------------------------------------------------------------
# metrics (fp64, on CPU copies) and small helpers
# ---------------------------------------------------------------------------------------------------
def rel_l2(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm() / (want.norm() + 1e-30))


def cosine(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


def rel_max(got, want):
    """max-abs error over max |want|."""
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def draw(rs, *shape):
    """fp32 standard normals of a numpy RandomState."""
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def bf16_bits(t):
    """fp32 -> the bf16 bit patterns (round-to-nearest-even) as int16."""
    return t.to(torch.bfloat16).view(torch.int16)


def from_bf16_bits(t):
    return t.view(torch.bfloat16).double()


def gpu_device(or_skip=False):
    """cuda:0.  A file marked gpu as a whole asserts that the GPU is there; ``or_skip`` is for a test that may be collected without one."""
    if or_skip and not torch.cuda.is_available():
        import pytest
        pytest.skip("needs a GPU")
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def load_npz(path):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def _rank_entry(fn, rank, world, port, args, q, backend="gloo"):
    """Child process of run_ranks: rendezvous on 127.0.0.1, run fn(rank, world, *args), report result or traceback."""
    import os
    import traceback
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    try:
        if backend == "nccl":               # RCCL: one rank per device; bind the communicator to the device up front
            import torch
            torch.cuda.set_device(rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        q.put((rank, "ok", fn(rank, world, *args)))
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))
    finally:
        q.close()
        q.join_thread()      # flush the result before leaving
        os._exit(0)          # no destroy_process_group: a peer that died must not leave this rank waiting in a collective


def run_ranks(fn, world, args=(), timeout=240, backend="gloo"):
    """Run fn(rank, world, *args) in `world` spawned processes over `backend` (gloo; "nccl" = RCCL, one rank per GPU); returns [result of rank 0, 1, ...].
    Never hangs: results are awaited with a deadline and every child is killed afterwards; a rank's exception is
    re-raised here with its traceback."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_entry, args=(fn, r, world, port, args, q, backend), daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    out, err = {}, None
    try:
        for _ in range(world):
            rank, status, payload = q.get(timeout=timeout)
            if status == "error":
                err = f"rank {rank} failed:\n{payload}"
                break
            out[rank] = payload
    except Exception as e:       # queue.Empty: a rank hung
        err = f"ranks did not finish within {timeout}s ({type(e).__name__}); finished: {sorted(out)}"
    finally:
        for p in procs:
            p.join(5)
            if p.is_alive():
                p.kill()
    assert err is None, err
    return [out[r] for r in range(world)]
