"""What the record reductions (sync, mov) share on the Python side: an array of records on the device and the number of
records a call produces."""
from ._device import DeviceArray as DeviceRecordArray   # noqa: F401  (`count` records of the subclass's `DTYPE`)
from .context import DeviceVec


def n_blocks(n, block):
    """records a call over n samples in blocks of `block` (0: one block) produces"""
    n, block = int(n), int(block)
    return -(-n // (block if block else max(n, 1)))


def _vec(ctx, x):
    return x if isinstance(x, DeviceVec) else ctx.vec(x)
