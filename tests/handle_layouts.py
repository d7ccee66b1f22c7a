"""Buffer layouts for one GP handle, and the bookkeeping that tells what a call wrote outside the region it may write.

include/mi_gp.h leaves the caller free to choose lda ("even, >= np"), an ldw of its own at every entry point that takes work
rows ("even and >= mi_gp_padded_n()"), the batch and work strides ("even, >= the matrix") and states no pointer alignment beyond
what an even leading dimension implies; it says nothing about what the buffers hold before the first call.  A ``Layout`` is one
point of that space: lda and ldw as functions of the padded capacity, the gap added to each stride, the element offset of every
pointer from the start of its allocation, and the fill of the whole allocation before first use.  ``Book`` allocates a handle's
buffers for a layout (on any backend: NumPy here, torch on the device), hands out the strided views and pointers, and after a call
reports every element outside the writable region -- the columns [capp, ld) of K, Z, W, the batch members and the work rows, the
gaps between members, the elements before the offset and behind the end -- whose bits are no longer the fill's.

Not a conftest and not a test module (and no torch at module level): tests/test_handle_layouts_host.py proves the table and that
the harness catches planted layout slips on a NumPy stand-in; tests/test_gpu_handle_sequences.py (RawHandle) and
tests/test_gpu_handle_layouts.py run the device."""
import numpy as np

NAN_BITS = 0x7FF80000DEADBEEF  # one quiet NaN with a payload: "unchanged" is a comparison of the int64 view
TAIL = 256                     # elements behind the end of every allocation of a poisoned layout


def padded(n):
    return (int(n) + 127) // 128 * 128


class Layout:
    """lda(capp), ldw(capp); gaps[kind] rows of the buffer's own ld added to the stride between batch members / work blocks
    (kind "K", "ZW", "work"); off_big / off_small elements between the allocation's start and the pointer (matrices and work
    buffers / vectors, points and outputs); fill "zeros" or "nan"."""

    def __init__(self, id, lda, ldw, gaps=(0, 0, 0), off_big=0, off_small=0, fill="nan"):
        self.id, self._lda, self._ldw = id, lda, ldw
        self.gaps = dict(zip(("K", "ZW", "work"), gaps))
        self.off_big, self.off_small, self.fill = off_big, off_small, fill
        self.tail = TAIL if fill == "nan" else 0

    def lda(self, capp):
        return self._lda(capp)

    def ldw(self, capp):
        return self._ldw(capp, self._lda(capp))

    def __repr__(self):
        return f"Layout({self.id})"


# tight: with handle_model.SIZES 100 and 700 np == capp == lda (cap 120 -> 128, cap 760 -> 768): no padding column at all
LAYOUTS = {ly.id: ly for ly in (
    Layout("default", lambda c: c + 16, lambda c, lda: lda, fill="zeros"),            # the harness as it was
    Layout("tight", lambda c: c, lambda c, lda: c),
    Layout("even", lambda c: c + 2, lambda c, lda: c + 6, gaps=(2, 2, 2)),           # ld % 4 == 2, ldw > lda
    Layout("wide", lambda c: c + 130, lambda c, lda: c, gaps=(4, 2, 6)),             # ldw < lda
    Layout("offset", lambda c: c + 16, lambda c, lda: c + 18, gaps=(2, 2, 2), off_big=2, off_small=1),
)}
DEFAULT = LAYOUTS["default"]
NON_DEFAULT = [k for k in LAYOUTS if k != "default"]


class Spec:
    """Geometry of one allocation: `count` members `stride` apart, each rows x ld with cols writable columns, starting `off`
    elements into `total`."""

    def __init__(self, name, off, count, rows, cols, ld, stride, tail):
        self.name, self.off, self.count, self.rows, self.cols, self.ld, self.stride = name, off, count, rows, cols, ld, stride
        self.total = off + (count - 1) * stride + rows * ld + tail

    def outside(self):
        """Flat indices of the elements the library may not write (ascending)."""
        inside = np.zeros(self.total, dtype=bool)
        for c in range(self.count):
            base = self.off + c * self.stride
            m = inside[base: base + self.rows * self.ld].reshape(self.rows, self.ld)
            m[:, : self.cols] = True
        return np.flatnonzero(~inside).astype(np.int64)

    def where(self, i):
        """A flat index in words."""
        if i < self.off:
            return f"element {i} of the allocation, {self.off - i} in front of the pointer"
        j = i - self.off
        c = min(j // self.stride, self.count - 1)
        r, col = divmod(j - c * self.stride, self.ld)
        if r >= self.rows:
            return f"element {i} of the allocation, {j - c * self.stride - self.rows * self.ld} behind member {c}'s last row"
        return f"member {c} row {r} column {col} (ld {self.ld}, writable columns [0, {self.cols}))"


class NumpyBackend:
    def alloc(self, total, bits):
        a = np.zeros(total)
        if bits is not None:
            a.view(np.int64)[:] = bits
        return a

    def bits(self, flat):
        return flat.view(np.int64)

    def index(self, idx):
        return idx

    def strided(self, flat, shape, strides, off):
        return np.lib.stride_tricks.as_strided(flat[off:], shape, [8 * s for s in strides])

    def any_changed(self, pairs, want):
        return [bool((b[i] != want).any()) for b, i in pairs]

    def first_changed(self, b, i, want):
        return int(i[np.flatnonzero(b[i] != want)[0]])


class Book:
    """The buffers of one handle under one layout."""

    def __init__(self, layout, capp, backend=None):
        self.layout, self.capp, self.be = layout, capp, backend or NumpyBackend()
        self.lda, self.ldw = layout.lda(capp), layout.ldw(capp)
        assert self.lda >= capp and self.ldw >= capp and self.lda % 2 == 0 and self.ldw % 2 == 0
        self.specs, self.flat, self._outside = {}, {}, {}
        self.checked = 0  # elements compared so far

    def _add(self, spec, shape, strides):
        self.specs[spec.name] = spec
        self.flat[spec.name] = self.be.alloc(spec.total, np.int64(NAN_BITS) if self.layout.fill == "nan" else None)
        return self.be.strided(self.flat[spec.name], shape, strides, spec.off)

    def matrix(self, name, rows, kind, count=None):
        """rows x ld (count members: count x rows x ld) with capp writable columns; kind "K" / "ZW" (ld = lda) or "work" (ldw)."""
        ld = self.ldw if kind == "work" else self.lda
        stride = (rows + self.layout.gaps[kind]) * ld
        assert stride % 2 == 0
        spec = Spec(name, self.layout.off_big, count or 1, rows, self.capp, ld, stride, self.layout.tail)
        if count is None:
            return self._add(spec, (rows, ld), (ld, 1))
        return self._add(spec, (count, rows, ld), (stride, ld, 1))

    def vector(self, name, length, big=False):
        """`length` contiguous elements (big: a work buffer or dense matrix at the matrices' offset)."""
        off = self.layout.off_big if big else self.layout.off_small
        return self._add(Spec(name, off, 1, 1, length, length, length, self.layout.tail), (length,), (1,))

    def stride(self, name):
        return self.specs[name].stride

    def violation(self):
        """None, or (buffer, flat index, text) of the first element outside a writable region whose bits changed."""
        if self.layout.fill != "nan":
            return None
        names = list(self.specs)
        for n in names:
            if n not in self._outside:
                self._outside[n] = self.be.index(self.specs[n].outside())
        pairs = [(self.be.bits(self.flat[n]), self._outside[n]) for n in names]
        self.checked += sum(len(i) for _, i in pairs)
        for n, (b, i), bad in zip(names, pairs, self.be.any_changed(pairs, NAN_BITS)):
            if bad:
                j = self.be.first_changed(b, i, NAN_BITS)
                return n, j, f"buffer {n}: {self.specs[n].where(j)} was written (layout {self.layout.id})"
        return None
