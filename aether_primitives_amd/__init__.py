"""aether_primitives_amd -- MI355X (gfx950) backend for the cf32 hot path of
razorheadfx/aether_primitives (VecOps / Fft / FIR / sampling).

The product is the C-ABI library `lib/libaether_hip.so` (include/aether_hip.h),
hand-written HIP.  This package is the thin host-side mirror of the reference's
Rust interface used by the tests and the bench: same names, same argument
meaning, same error behaviour (length mismatches raise, as the reference
panics).  Nothing here computes on the CPU; without the built library the
import fails.
"""
from ._lib import AetherError, LengthMismatch, load as _load

_load()   # fail loudly at import time if the HIP library is not built

from .context import (Context, DeviceVec, DeviceF32, DeviceF64, HostVec, VecStats,  # noqa: E402
                      LEVEL_NORM, LEVEL_DB, LEVEL_POWER_DB)
from .fft import Scale, HipFft, SIGN_REF_FWD, SIGN_REF_BWD  # noqa: E402
from .fir import Fir                                      # noqa: E402
from .corr import Corr, CorrPeak                          # noqa: E402
from . import sampling                                    # noqa: E402
from . import modulation                                  # noqa: E402
from . import noise                                       # noqa: E402
from . import sequence                                    # noqa: E402
from .sequence import Sequence, lte_gold                  # noqa: E402
from . import chan                                        # noqa: E402
from .chan import Channelizer                             # noqa: E402
from . import synth                                       # noqa: E402
from .synth import Synthesizer                            # noqa: E402
from . import resamp                                      # noqa: E402
from .resamp import Resampler                             # noqa: E402
from . import arb                                         # noqa: E402
from .arb import ArbResampler, step_word                  # noqa: E402
from . import nco                                         # noqa: E402
from .nco import Nco                                      # noqa: E402
from . import sync                                        # noqa: E402
from . import mov                                         # noqa: E402
from . import cc                                          # noqa: E402
from .cc import ConvCode                                  # noqa: E402
from . import remap                                       # noqa: E402
from .remap import Remap                                  # noqa: E402
from . import crc                                         # noqa: E402
from .crc import Crc, DeviceU64, pack_bits, unpack_bits   # noqa: E402
from . import ldpc                                        # noqa: E402
from .ldpc import Ldpc                                    # noqa: E402
from . import rs                                          # noqa: E402
from .rs import Rs                                        # noqa: E402
from . import polar                                       # noqa: E402
from .polar import Polar, PolarList                         # noqa: E402
from . import turbo                                       # noqa: E402
from .turbo import Turbo                                  # noqa: E402
from . import ofdm                                        # noqa: E402
from .ofdm import Ofdm                                    # noqa: E402
from .modulation import DeviceBits, DeviceSoft            # noqa: E402
from . import file                                        # noqa: E402
from . import pool                                        # noqa: E402
from . import pipeline                                    # noqa: E402
from .evm import assert_evm, evm_db                       # noqa: E402

__all__ = ["AetherError", "LengthMismatch", "Context", "DeviceVec", "DeviceF32", "DeviceF64", "HostVec", "VecStats", "LEVEL_NORM",
           "LEVEL_DB", "LEVEL_POWER_DB", "Scale", "HipFft",
           "SIGN_REF_FWD", "SIGN_REF_BWD", "Fir", "Corr", "CorrPeak", "sampling", "modulation", "noise", "sequence", "Sequence",
           "lte_gold", "chan", "Channelizer", "synth", "Synthesizer", "resamp", "Resampler", "arb", "ArbResampler", "step_word",
           "nco", "Nco", "sync", "mov", "cc", "ConvCode", "remap", "Remap", "crc", "Crc", "DeviceU64", "pack_bits", "unpack_bits", "ldpc", "Ldpc", "rs", "Rs", "polar", "Polar", "PolarList", "turbo", "Turbo", "ofdm", "Ofdm", "DeviceBits", "DeviceSoft",
           "assert_evm", "evm_db"]
