"""Time zone rules (include/orcg.h orcg_timezone_*; the reference's Timezone,
c++/src/Timezone.hh). Host only: no GPU is touched."""
import collections
import ctypes

from . import _lib
from ._lib import check

Variant = collections.namedtuple("Variant", "gmt_offset is_dst name")  # TimezoneVariant


class Timezone:
    """One zone's rules: TZif transitions plus the POSIX rule for the future."""

    def __init__(self, handle, name):
        self._L = _lib.load()
        self._h = handle
        self.name = name

    @classmethod
    def _make(cls, call, name):
        L = _lib.load()
        h = ctypes.c_void_p()
        check(call(L, ctypes.byref(h)), L.orcg_timezone_last_error)
        return cls(h, name)

    @classmethod
    def parse(cls, name, data):
        """getTimezone(filename, bytes): TZif v1 / v2+ bytes; a bad file raises
        ParseError with the reference's TimezoneError text."""
        data = bytes(data)
        return cls._make(lambda L, out: L.orcg_timezone_parse(name.encode(), data, len(data), out), name)

    @classmethod
    def load(cls, name):
        """getTimezoneByName: aliases, then $TZDIR (else $CONDA_PREFIX/share/
        zoneinfo, else /usr/share/zoneinfo); InvalidArgument if not found."""
        return cls._make(lambda L, out: L.orcg_timezone_load(name.encode(), out), name)

    def close(self):
        if self._h:
            self._L.orcg_timezone_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def version(self):
        return int(self._L.orcg_timezone_version(self._h))

    def epoch(self):
        """Timezone::getEpoch: 2015-01-01 00:00:00 in this zone."""
        return int(self._L.orcg_timezone_epoch(self._h))

    def variant(self, clk):
        """Timezone::getVariant(clk)."""
        off, dst, name = ctypes.c_int64(), ctypes.c_int(), ctypes.c_char_p()
        check(self._L.orcg_timezone_variant(self._h, int(clk), ctypes.byref(off), ctypes.byref(dst),
                                            ctypes.byref(name)))
        return Variant(off.value, bool(dst.value), (name.value or b"").decode(errors="replace"))

    def convert_to_utc(self, clk):
        return int(self._L.orcg_timezone_convert_to_utc(self._h, int(clk)))

    def convert_from_utc(self, clk):
        return int(self._L.orcg_timezone_convert_from_utc(self._h, int(clk)))
