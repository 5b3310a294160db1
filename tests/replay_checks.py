"""What the GPU tests of the five fused replay entry points share: every slot of a schedule as a single _dev call, the
same slots in one call, and the byte comparison of the two.

A test file describes its entry point as a Family and its schedule as an object `inp` with
  inp.kinds        the kind of every slot, uint8 (all zero where the entry point has one kind only)
  inp.T            tags in the bank
  inp.d_r          a device tensor (its device is where the outputs go)
  inp.bank(chunk)  a fresh handle, created under KFPOS_TRACE_CHUNK_STEPS=chunk
and everything its own Family's callables read. torch is imported where a GPU is used, not on import."""
import contextlib
import os

import numpy as np


@contextlib.contextmanager
def env(**kv):
    """environment variables the library reads in kfpos_create; None unsets"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def up(a, dev="cuda:0"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ordinals(kinds, n_kinds):
    """-> (e, kind, how many slots of that kind came before e) for every slot e"""
    n = [0] * n_kinds
    for e, kind in enumerate(kinds):
        yield e, int(kind), n[kind]
        n[kind] += 1


def same_bytes(got, ref, names, what, first=0):
    for g, r, name in list(zip(got, ref, names))[first:]:
        assert g.shape == r.shape and g.dtype == r.dtype, (what, name)
        assert g.tobytes() == r.tobytes(), (what, name)


class Family:
    """what differs between the entry points:
    names    what the entries of a result are called: position and status of every slot, then what final() returns
    n_kinds  how many kinds of slot there are
    dts(inp) the schedule's own dt of every slot: a host array of scalars, or a device tensor with a row per slot
    final(b) the bank's state after a run, a tuple of arrays
    position(b) -> (3, T)
    single(b, inp, e, kind, ordinal, status_row, stream, dt)   slot e as one _dev call; dt is dts[e]
    call(b, inp, n, dts, traj, status_events, status, stream)  the first n slots in one call"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def single_calls(fam, b, inp, dts=None, n_slots=None):
    """the (first n_slots) slots as single _dev calls -> (position after every slot, status of every slot) + final"""
    import torch
    dts = fam.dts(inp) if dts is None else dts
    n, nt = n_slots or inp.kinds.size, inp.T
    st = torch.full((n, nt), -2, dtype=torch.int32, device=inp.d_r.device)   # (not one_call's fill: no word is left)
    stream = torch.cuda.current_stream().cuda_stream
    traj = np.zeros((n, 3, nt))
    for e, kind, i in ordinals(inp.kinds[:n], fam.n_kinds):
        fam.single(b, inp, e, kind, i, st[e], stream, dts[e])
        torch.cuda.synchronize()
        traj[e] = fam.position(b)
    return (traj, st.cpu().numpy()) + fam.final(b)


def one_call(fam, b, inp, outputs=True, dts=None, n_slots=None):
    """the same slots in one call; outputs=False: trajectory = status_events = NULL -> (None, status) + final"""
    import torch
    dts = fam.dts(inp) if dts is None else dts
    n, nt, dev = n_slots or inp.kinds.size, inp.T, inp.d_r.device
    traj = torch.full((n, 3, nt), 7.0, dtype=torch.float64, device=dev) if outputs else None
    ste = torch.full((n, nt), -1, dtype=torch.int32, device=dev) if outputs else None
    st = torch.full((nt,), -1, dtype=torch.int32, device=dev)
    fam.call(b, inp, n, dts[:n], traj, ste, st, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    last = st.cpu().numpy()
    if not outputs:
        return (None, last) + fam.final(b)
    assert np.array_equal(last, ste[-1].cpu().numpy()), "status is not the last slot's"
    return (traj.cpu().numpy(), ste.cpu().numpy()) + fam.final(b)


def check_one_call(fam, inp, what, prepare=None, chunks=(None, 7), dts=None, n_slots=None):
    """single calls against one call per launch size, and once (at the last size) with trajectory = status_events =
    NULL; prepare(b) runs on every fresh handle first -> what the single calls gave"""
    def bank(chunk=None):
        b = inp.bank(chunk)
        if prepare:
            prepare(b)
        return b

    b = bank()
    ref = single_calls(fam, b, inp, dts, n_slots)
    b.close()
    for chunk in chunks:
        b = bank(chunk)
        got = one_call(fam, b, inp, dts=dts, n_slots=n_slots)
        b.close()
        same_bytes(got, ref, fam.names, f"{what} chunk={chunk}")
    b = bank(chunks[-1])
    bare = one_call(fam, b, inp, outputs=False, dts=dts, n_slots=n_slots)
    b.close()
    assert bare[1].tobytes() == ref[1][-1].tobytes(), (what, "last status")
    same_bytes(bare, ref, fam.names, f"{what} without per-slot outputs", first=2)
    return ref
