"""Device buffers at a chosen address residue (mod 16) between guard bytes: what tests/test_gpu_dev_pointer_alignment.py
hands to the `_dev` entry points instead of the start of a fresh allocation.  `shifted` returns a uint8 view whose
data_ptr() % 16 is the residue asked for, with `guard` bytes of `fill` in front of it and behind it inside the same
allocation; `guards_intact` says after a call whether both are still there, i.e. whether nothing was written in front of or
behind the caller's range.  (Reads outside the range cannot be seen this way.)"""
import numpy as np

ALIGN = 16


def shifted(nbytes, residue, guard=64, fill=0xA5):
    """uint8 CUDA view of `nbytes` bytes at an address = residue (mod 16), every byte of the allocation set to `fill`"""
    import torch
    assert 0 <= residue < ALIGN and guard >= 0 and nbytes >= 0
    buf = torch.full((guard + ALIGN + nbytes + guard + ALIGN,), fill, dtype=torch.uint8, device="cuda")
    start = guard + (residue - (buf.data_ptr() + guard)) % ALIGN
    view = buf[start:start + nbytes]
    assert view.data_ptr() % ALIGN == residue and start >= guard and start + nbytes + guard <= buf.numel()
    view._dev_shift = (buf, start, nbytes, guard, fill)
    return view


def shifted_from(data, residue, guard=64, fill=0xA5):
    """`shifted` holding a copy of `data` (bytes or a numpy array, viewed as bytes)"""
    import torch
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    view = shifted(len(a), residue, guard, fill)
    if len(a):
        view.copy_(torch.from_numpy(a.copy()))
    return view


def guards_intact(view):
    """both guard regions of a `shifted` view still hold the fill byte"""
    import torch
    torch.cuda.synchronize()
    buf, start, nbytes, guard, fill = view._dev_shift
    front, back = buf[start - guard:start], buf[start + nbytes:start + nbytes + guard]
    return bool((front == fill).all()) and bool((back == fill).all())

