"""Plane layouts for the layout tests (tests/test_gpu_layouts.py, tests/test_layouts.py): planes carved out of a filled arena at a chosen
pitch and base-address residue, the check that every byte that is not a sample still holds the fill, and the tables of named layouts that
include/mvtools_amd.h ("Plane layouts") allows.  Test infrastructure; imports without a GPU and works on device="cpu" tensors."""
import numpy as np
import torch

FILLS = (0xA5, 0x5A)
NAN_FILL = bytes([0x00, 0x00, 0xC0, 0x7F])  # the float32 quiet NaN, little endian; float planes only
REGIONS = ("before the plane", "row tails", "rows after the plane", "beyond")


def ceil_to(n, a):
    return (n + a - 1) // a * a


def _pattern(fill, first_address, n, device):
    """n fill bytes as they lie at first_address: a byte value, or a byte string repeated from address 0 (so that a 4-byte pattern falls on
    whole float32 samples wherever a plane starts at a multiple of 4)"""
    if isinstance(fill, int):
        return torch.full((n,), fill, dtype=torch.uint8, device=device)
    pat = np.frombuffer(bytes(fill), dtype=np.uint8)
    idx = (np.arange(n, dtype=np.int64) + first_address % len(pat)) % len(pat)
    return torch.from_numpy(pat[idx].copy()).to(device)


def carve(shape_rows, row_bytes, pitch, base_residue, fill, guard_rows=8, guard_bytes=256, device="cuda"):
    """(arena, view): ONE uint8 tensor filled with `fill` and a [shape_rows, pitch] view into it with view.data_ptr() % 256 == base_residue and
    view.stride(0) == pitch.  guard_rows rows of pitch bytes above and below the plane and at least guard_bytes bytes beyond them belong to the
    arena: an over-read or over-write of a few vectors stays inside memory the test owns and shows up as a changed guard byte (intact).  The
    view covers rows * pitch bytes, the whole last row also at a tight pitch."""
    assert pitch >= row_bytes > 0 and shape_rows > 0 and 0 <= base_residue < 256
    body = shape_rows * pitch
    lead = guard_bytes + guard_rows * pitch
    total = lead + 256 + body + guard_rows * pitch + guard_bytes
    arena = torch.empty(total, dtype=torch.uint8, device=device)
    arena.copy_(_pattern(fill, arena.data_ptr(), total, device))
    start = lead + (base_residue - (arena.data_ptr() + lead)) % 256
    view = arena[start:start + body].view(shape_rows, pitch)
    assert view.data_ptr() % 256 == base_residue and view.stride(0) == pitch and view.data_ptr() - arena.data_ptr() == start
    return arena, view


def intact(arena, view, row_bytes, fill, guard_rows=8):
    """the damaged regions among REGIONS, as (region, row, column, value) of the first damaged byte of each -- row and column count from the
    plane's first sample in units of its pitch and of bytes (negative rows lie before the plane).  [] when every byte of the arena that is
    not one of the view's rows x row_bytes samples still holds the fill."""
    rows, pitch = view.shape
    start = view.data_ptr() - arena.data_ptr()
    end = start + rows * pitch
    want = _pattern(fill, arena.data_ptr(), arena.numel(), arena.device)
    bad = (arena != want)
    bad[start:end].view(rows, pitch)[:, :row_bytes] = False
    if not bool(bad.any()):
        return []
    idx = torch.nonzero(bad).flatten().cpu().numpy()
    after = end + guard_rows * pitch
    out = []
    for name, sel in ((REGIONS[0], idx < start), (REGIONS[1], (idx >= start) & (idx < end)), (REGIONS[2], (idx >= end) & (idx < after)),
                      (REGIONS[3], idx >= after)):
        if sel.any():
            i = int(idx[sel][0])
            out.append((name, (i - start) // pitch, (i - start) % pitch, int(arena[i])))
    return out


def describe(damage):
    return "; ".join("%s: first damaged byte at row %d, column %d (now 0x%02x)" % d for d in damage)


def put(view, arr):
    """the numpy plane arr (rows x width samples of any type) into the samples of view"""
    a = np.ascontiguousarray(arr)
    raw = a.view(np.uint8).reshape(a.shape[0], -1)
    view[:, :raw.shape[1]] = torch.from_numpy(raw).to(view.device)


def get(view, width, dtype):
    """the rows x width samples of view as a numpy plane"""
    n = width * np.dtype(dtype).itemsize
    return view[:, :n].contiguous().cpu().numpy().view(dtype).reshape(view.shape[0], width)


# ---- clip-side planes of w samples of bps bytes: (pitch, residue) per plane in bytes.  `row` = w * bps, `pad` = row rounded up to 256; the
# extra bytes and the residue are given in samples so that every layout is legal for its sample size (float: multiples of 4).
#   name        pitch base  + samples  + bytes   residue (samples)   V's pitch + bytes
CLIP_LAYOUTS = {
    "padded":    ("pad", 0, 0, 0, 0),      # the control: what every other GPU test uses
    "tight":     ("row", 0, 0, 0, 0),
    "plus1":     ("row", 1, 0, 0, 0),      # odd for 8 bit, 2 mod 4 for 16 bit whenever w is even
    "offset":    ("pad", 0, 256, 1, 0),    # a plane inside a wider frame, one sample off a 256-byte boundary
    "offset3":   ("pad", 0, 256, 3, 0),    # ... three samples off
    "uv_differ": ("pad", 0, 0, 0, 256),    # V rows 256 bytes longer than U rows: only where the header does not require equal chroma pitches
}


def clip_layout(name, w, bps, plane=0):
    """(pitch, base residue) in bytes of plane `plane` (0 Y, 1 U, 2 V) of w samples in the named layout"""
    base, samples, extra, residue, v_extra = CLIP_LAYOUTS[name]
    row = w * bps
    pitch = (ceil_to(row, 256) if base == "pad" else row) + samples * bps + extra + (v_extra if plane == 2 else 0)
    return pitch, residue * bps


def clip_planes(name, widths, heights, bps, fill, device="cuda"):
    """a frame in the named layout: per plane (arena, view)"""
    out = []
    for p, (w, h) in enumerate(zip(widths, heights)):
        pitch, residue = clip_layout(name, w, bps, p)
        out.append(carve(h, w * bps, pitch, residue, fill, device=device))
    return out


# ---- super planes: pitches that are multiples of 16 but not of 256, planes on 16-byte but not 256-byte boundaries
#   name       rounding  + bytes (sup16: + 32 where that makes the number of 16-byte units odd)   residue
SUPER_LAYOUTS = {
    "sup16":  (16, 16, 16),
    "sup256": (256, 16, 48),
}


def super_pitch(name, row_bytes):
    unit, extra, _ = SUPER_LAYOUTS[name]
    pitch = ceil_to(row_bytes, unit) + extra
    if name == "sup16" and (pitch // 16) % 2 == 0:
        pitch += 16
    return pitch


def super_residue(name):
    return SUPER_LAYOUTS[name][2]
