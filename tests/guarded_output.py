"""A kernel output the harnesses can trust: the body sits between two 64-byte
guards of 0xa5 (64 keeps the 16-byte alignment the kernels' vector stores
assume) and is poisoned before the launch - with `expect ^ 0x80` byte by byte
when the reference is known, so that a byte the kernel does not write is wrong
with certainty, else with 0xa5.  download() asserts both guards intact, then
returns the body.
"""
import numpy as np

GUARD = 64
FILL = 0xa5


class GuardedOutput:
    def __init__(self, nbytes, expect=None):
        from band_amd.device import DeviceBuffer
        self.nbytes = int(nbytes)
        host = np.full(self.nbytes + 2 * GUARD, FILL, np.uint8)
        if expect is not None:
            ref = np.ascontiguousarray(expect).reshape(-1).view(np.uint8)
            assert ref.size == self.nbytes, "expect holds %d bytes, the output %d" % (ref.size, self.nbytes)
            host[GUARD:GUARD + self.nbytes] = ref ^ 0x80
        self.buf = DeviceBuffer.from_array(host)

    @property
    def value(self):
        """the body's device address: what the kernel is given"""
        return self.buf.value + GUARD

    def download(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        raw = self.buf.download(np.uint8, (self.nbytes + 2 * GUARD,))
        for side, guard in (("in front of", raw[:GUARD]), ("behind", raw[GUARD + self.nbytes:])):
            hit = np.flatnonzero(guard != FILL)
            assert hit.size == 0, "the kernel wrote %s its output: %d guard bytes changed, the first at guard offset %d" % (
                side, hit.size, hit[0])
        return raw[GUARD:GUARD + out.nbytes].view(out.dtype).reshape(shape).copy()

    def free(self):
        self.buf.free()
