"""gdn_amd — MI355X-native (gfx950) implementation of GDN's graph-attention hot path behind
the reference's `GDN(nn.Module).forward(data, org_edge_index)` API (models/GDN.py:82-187)."""
from .model import GDN, GNNLayer, GraphLayer, OutLayer  # noqa: F401

__all__ = ["GDN", "GNNLayer", "GraphLayer", "OutLayer", "Prep", "PrepUnits"]


def __getattr__(name):
    # gdn_amd.Prep, imported on first use: `python -m gdn_amd.prep` then runs a module the package has not imported yet
    if name == "Prep":
        from .prep import Prep
        return Prep
    if name == "PrepUnits":
        from .prep import PrepUnits
        return PrepUnits
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
