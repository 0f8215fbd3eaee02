"""The data path.  The room simulator's names (dataset/rir.py) are reachable from here; they are looked up on first
use, so importing the package still loads nothing."""
__all__ = ["shoebox_rir", "beta_from_t60", "draw_rooms", "Rooms"]


def __getattr__(name):
    if name in __all__:
        from . import rir
        return getattr(rir, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
