"""CPU-only: the guarded buffer every emulator test relies on to say that no byte outside a buffer was written (emu_lib.Guarded): one
byte written immediately before or immediately after its bytes is seen."""
import pytest

from emu_lib import GUARD, Guarded


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_intact_sees_one_byte_on_either_side(n):
    g = Guarded(n, fill=0xA7)
    assert g.a.size == g.n == n and g.ptr % 256 == 0 and g.ptr == g.store.ctypes.data + g.lead
    assert g.intact()
    g.a[:] = GUARD ^ 0xFF                                    # the buffer's own bytes are the caller's
    assert g.intact()
    for at in (g.lead - 1, g.lead + n):                      # immediately before `a`, immediately after it
        keep = g.store[at]
        g.store[at] = keep ^ 0x01
        assert not g.intact(), at
        g.store[at] = keep
        assert g.intact()
    for at in (0, g.store.size - 1):                         # the far ends of the guard bytes
        g.store[at] ^= 0x80
        assert not g.intact(), at
        g.store[at] ^= 0x80
    assert g.intact()
