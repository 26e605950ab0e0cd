"""Host-only table of what the library decides per shape (no GPU needed): one line per shape of a fixed grid with
every host query of the C ABI, and, when the library has gdn_kernel_family, the kernel family of every stage
(include/gdn_hip.h "route table").  Two builds decide alike exactly when the columns they share are identical line
for line:  python tools/route_grid.py > grid.txt  on each, then diff."""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdn_amd import _lib  # noqa: E402

NS = (1, 20, 127, 128, 300, 610, 700, 2200, 4096)
WS = (1, 8, 16, 32, 33, 64, 65, 1024)
DS = (8, 16, 24, 32, 64, 128, 256)
KS = (1, 15, 16, 30, 63, 64)
BATCH = 3
STAGES = ("project", "aggregate", "attn_bwd", "project_bwd", "terms", "head", "fused")


def shapes():
    return [s for s in itertools.product(NS, WS, DS, KS) if s[3] <= s[0]]


def main():
    lib = ctypes.CDLL(_lib.LIB_PATH)      # (not _lib.load(): the table is also taken from builds of another ABI)
    for name in ("gdn_attn_aggregate_bwd_workspace_bytes", "gdn_project_bwd_workspace_bytes", "gdn_fused_plan_bytes"):
        getattr(lib, name).restype = ctypes.c_longlong
    family = getattr(lib, "gdn_kernel_family", None)
    for n, w, d, k in shapes():
        line = (f"n={n} w={w} d={d} k={k} tile_fits={lib.gdn_tile_fits(n, w, d, k)} "
                f"train={lib.gdn_train_supported(n, w, d, k)} reverse={lib.gdn_attn_aggregate_bwd_uses_reverse(n, d, k)} "
                f"attn_bwd_ws={lib.gdn_attn_aggregate_bwd_workspace_bytes(BATCH, n, d, k)} "
                f"project_bwd_ws={lib.gdn_project_bwd_workspace_bytes(n, w, d)} "
                f"plan={lib.gdn_fused_plan_bytes(n, w, d, k, 0)} plan_bf16={lib.gdn_fused_plan_bytes(n, w, d, k, 1)} "
                f"terms_pitch={lib.gdn_terms_pitch(w)}")
        if family is not None:
            line += " |" + "".join(f" {s}={family(i, n, w, d, k, 0)}" for i, s in enumerate(STAGES))
        print(line)


if __name__ == "__main__":
    main()
