"""Guarded buffers: the bounds checker of this suite ("Memory contract").

The C ABI works on caller-owned buffers, and every product caller sizes them exactly out of a caching allocator, so a
kernel that writes past an extent, or reads past one, lands in a neighbouring live tensor: no fault and no wrong value in
the tensor a parity test looks at.  `guarded()` puts a buffer between two bands of a known byte pattern inside ONE flat
uint8 allocation, `check()` compares the bands (and the pitch gaps of a strided view) with the pattern on the device.

    [ front band | payload (rows x pitch, the last row only `width` wide) | back band ]

Band size is a condition: at least 64 KiB and at least 256 rows at the buffer's pitch (the largest tile of any kernel
here is 256 rows: big-tile GEMM 256 x 256/128, ring GEMM 128 x 128, edge-chain groups 64-128 edge rows), so an overrun by
a whole ragged tile still lands inside a band.  Works on CPU tensors too (tests/test_guarded.py, the host seed generator).
"""
import numpy as np
import torch

MIN_BAND = 64 * 1024
TILE_ROWS = 256


class GuardDamage(AssertionError):
    """check() found bytes that differ from the band pattern; .reports = list of dicts (side, first, last, count)."""

    def __init__(self, text, reports):
        super().__init__(text)
        self.reports = reports


class Guarded:
    def __init__(self, shape, dtype, pitch=None, align=512, offset=0, band_fill=0xFF, device="cpu", tile_row_bytes=None,
                 name="buffer"):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        assert len(shape) >= 1 and all(s >= 0 for s in shape)
        assert band_fill in (0xFF, 0x00), "two patterns: 0xFF (NaN as f16/f32/f64, -1 as int32/int64) and 0x00"
        self.name, self.shape, self.dtype, self.band_fill = name, shape, dtype, band_fill
        self.esize = torch.empty((), dtype=dtype).element_size()
        self.width = shape[-1]
        self.rows = int(np.prod(shape[:-1], dtype=np.int64)) if len(shape) > 1 else 1
        self.pitch = self.width if pitch is None else int(pitch)
        assert self.pitch >= self.width, "pitch %d < width %d" % (self.pitch, self.width)
        assert len(shape) > 1 or self.pitch == self.width, "a 1-D buffer has no pitch"
        assert align >= 1 and 0 <= offset < align and offset % self.esize == 0, "offset must keep the element type aligned"
        self.align, self.offset = align, offset
        # the payload spans whole pitches up to the last row, which is only `width` wide: the gap after it belongs to the back band
        span_elems = (self.rows - 1) * self.pitch + self.width if self.rows > 0 and self.width > 0 else 0
        self.span = span_elems * self.esize
        row_bytes = self.pitch * self.esize if len(shape) > 1 else self.esize
        self.band = max(MIN_BAND, TILE_ROWS * max(row_bytes, tile_row_bytes or 0))
        self.raw = torch.empty(self.band + self.span + self.band + align + self.esize, dtype=torch.uint8, device=device)
        self.raw.fill_(band_fill)
        base = self.raw.data_ptr() + self.band
        self.p0 = self.band + (offset - base) % align                    # payload start inside raw: address == offset (mod align)
        self.p1 = self.p0 + self.span
        assert (self.raw.data_ptr() + self.p0) % align == offset
        flat = self.raw[self.p0:self.p1].view(dtype)
        strides = []
        s = self.pitch
        for dim in reversed(shape[:-1]):
            strides.append(s)
            s *= dim
        strides = tuple(reversed(strides)) + (1,)
        self.t = torch.as_strided(flat, shape, strides) if span_elems else torch.empty(shape, dtype=dtype, device=device)
        gap = (self.pitch - self.width) * self.esize
        self._gaps = None
        if gap and self.rows > 1:
            self._gaps = torch.as_strided(self.raw, (self.rows - 1, gap), (self.pitch * self.esize, 1), self.p0 + self.width * self.esize)

    # ------------------------------------------------------------------ payload
    def fill_payload_bytes(self, value):
        """Every byte of the declared extent (not the pitch gaps) = value."""
        if self.span:
            rowsv = torch.as_strided(self.raw, (self.rows, self.width * self.esize), (self.pitch * self.esize, 1), self.p0)
            rowsv.fill_(value)
        return self

    def set(self, src):
        self.t.copy_(torch.as_tensor(src).reshape(self.shape))
        return self

    def refill_guards(self, band_fill):
        """Switch the pattern of the bands and pitch gaps; the payload keeps its content."""
        assert band_fill in (0xFF, 0x00)
        self.band_fill = band_fill
        self.raw[:self.p0].fill_(band_fill)
        self.raw[self.p1:].fill_(band_fill)
        if self._gaps is not None:
            self._gaps.fill_(band_fill)
        return self

    def payload_bits(self):
        """The declared extent as a compact uint8 tensor [rows, width*esize] (a copy): bitwise comparisons, NaN-safe."""
        if not self.span:
            return torch.empty((0,), dtype=torch.uint8, device=self.raw.device)
        return torch.as_strided(self.raw, (self.rows, self.width * self.esize), (self.pitch * self.esize, 1), self.p0).clone()

    # ------------------------------------------------------------------ guards
    def _damaged(self):
        """Number of damaged guard bytes, one device reduction per region, no copy of the buffer."""
        f = self.band_fill
        n = torch.count_nonzero(self.raw[:self.p0] != f) + torch.count_nonzero(self.raw[self.p1:] != f)
        if self._gaps is not None:
            n = n + torch.count_nonzero(self._gaps != f)
        return n

    def reports(self):
        """Damage per side: offsets are bytes relative to the payload's first byte (front: negative; back: >= span)."""
        f, out = self.band_fill, []

        def add(side, idx, origin):
            if idx.numel():
                out.append({"buffer": self.name, "side": side, "first": int(idx.min().item()) + origin,
                            "last": int(idx.max().item()) + origin, "count": int(idx.numel())})

        add("front", torch.nonzero(self.raw[:self.p0] != f).flatten(), -self.p0)
        add("back", torch.nonzero(self.raw[self.p1:] != f).flatten(), self.span)
        if self._gaps is not None:
            rc = torch.nonzero(self._gaps != f)
            if rc.numel():
                add("gap", rc[:, 0] * (self.pitch * self.esize) + self.width * self.esize + rc[:, 1], 0)
        return out

    def check(self):
        if int(self._damaged().item()) == 0:
            return
        reps = self.reports()
        text = "; ".join("%s: %s band damaged, %d bytes, offsets %d..%d relative to the payload (%d bytes, pitch %d x %d B)"
                         % (r["buffer"], r["side"], r["count"], r["first"], r["last"], self.span, self.pitch, self.esize) for r in reps)
        raise GuardDamage(text, reps)


def guarded(shape, dtype, *, pitch=None, align=512, offset=0, band_fill=0xFF, device="cpu", tile_row_bytes=None, name="buffer"):
    """One flat uint8 allocation [front band | payload | back band]; .t is the (possibly pitched) view of the payload whose
    base address is `offset` (mod `align`); .check() raises GuardDamage naming side, first/last byte offset and count."""
    return Guarded(shape, dtype, pitch=pitch, align=align, offset=offset, band_fill=band_fill, device=device,
                   tile_row_bytes=tile_row_bytes, name=name)


class Arena:
    """The buffers of one call.  mode "guard": inputs, outputs and workspaces are guarded buffers (inputs' bands and the
    workspaces' content = `fill`, outputs pre-filled 0xFF = NaN / -1).  mode "compact": the way the parity tests call —
    allocator-aligned compact tensors, pitch == width, zeroed workspaces."""

    def __init__(self, mode, fill=0xFF, device="cpu"):
        assert mode in ("guard", "compact")
        self.mode, self.fill, self.device = mode, fill, device
        self.bufs, self.outs, self.wss = [], [], []

    @property
    def compact(self):
        return self.mode == "compact"

    def _make(self, shape, dtype, pitch, offset, fill, name, tile_row_bytes=None):
        if self.compact:
            pitch, offset = None, 0
        g = guarded(shape, dtype, pitch=pitch, offset=offset, band_fill=fill, device=self.device, name=name, tile_row_bytes=tile_row_bytes)
        if not self.compact:
            self.bufs.append(g)
        return g

    def inp(self, arr, pitch=None, offset=0, name="input"):
        arr = torch.as_tensor(np.ascontiguousarray(arr)) if not torch.is_tensor(arr) else arr
        g = self._make(arr.shape, arr.dtype, pitch, offset, self.fill, name)
        g.set(arr.to(self.device))
        return g.t

    def out(self, shape, dtype=torch.float32, pitch=None, offset=0, name="output"):
        g = self._make(shape, dtype, pitch, offset, 0xFF, name)
        g.fill_payload_bytes(0xFF)
        self.outs.append(g)
        return g.t

    def ws(self, nbytes, offset=0, tile_row_bytes=None, name="workspace"):
        g = self._make((int(nbytes),), torch.uint8, None, offset, 0xFF if self.compact else self.fill, name, tile_row_bytes)
        g.fill_payload_bytes(0x00 if self.compact else self.fill)
        self.wss.append(g)
        return g.t

    def refill_outputs(self):
        for g in self.outs:
            g.fill_payload_bytes(0xFF)

    def check(self):
        for g in self.bufs:
            g.check()
