"""The forward plan's rules ("The forward plan") in plain Python: what ``mgs_debug_forward_plan`` must answer.
Written from the table there, not from the C++.  ``opt``: the debug options that are set (absent or negative = default).
``banded_bytes`` / ``two_pass_bytes``: the two scratch sizes the banded decision compares -- the sort's own arithmetic, taken as
given."""
ONE_SWEEP_MAX, FORCED_MIN = 512 * 1024, 64 * 1024         # a sort above 512 k pairs takes counted tiles; the knob forces > 64 k
EXCLUSIVE_DEVICE = 1                                      # MGS_FLAG_EXCLUSIVE_DEVICE


def plan(P, W, H, flags, R, capacity, opt, banded_bytes, two_pass_bytes):
    o = lambda name, default: opt[name] if opt.get(name, -1) >= 0 else default  # noqa: E731
    knob = o("radix_scanned", -1)
    large = (lambda n: knob == 1) if knob >= 0 else (lambda n: n > ONE_SWEEP_MAX)         # the forward's "large map"
    counted = lambda n: large(n) and (knob < 0 or n > FORCED_MIN)  # noqa: E731            the sort's counted-tiles path
    p = dict(p=P, w=W, h=H, flags=flags, capacity_mode=int(capacity))
    p["tiles_x"], p["tiles_y"] = (W + 15) // 16, (H + 15) // 16
    nt = p["ntiles"] = p["tiles_x"] * p["tiles_y"]
    tb = p["tile_bits"] = max(1, (nt - 1).bit_length())
    p["small_grid"] = int(nt <= 65536)
    lo = max(tb - 5, 0)                                   # depth bits that do not fit beside the tile id
    pt = p["per_tile"] = int(P > 0 and large(P) and tb <= 16 and P <= 1 << (32 - lo))
    items = p["scan_items"] = 256 if pt and o("pre_scan", 1) != 0 else 2048
    p["scan_shift"], p["scan_blocks"] = items.bit_length() - 1, -(-P // items)
    p["scan_small"] = int(P > 0 and items == 2048 and o("scan_small", 1) != 0 and p["scan_blocks"] <= 64)
    nb = -(-nt // 256)
    counted_bands = p["bands_counted"] = nb if o("tile_sort_banded", 1) != 0 and items == 256 and tb > 8 and nb <= 32 else 0
    p["rect_packed"] = int(not pt and P > 0 and counted(P) and p["tiles_x"] <= 255 and p["tiles_y"] <= 255)
    p["exclusive"] = int(flags & EXCLUSIVE_DEVICE != 0)
    R = p["r"] = 0 if P == 0 else R
    p["r_cap"] = R if capacity else (0xFFFFFFFF if R > 0 else 0)
    dsm = o("dup_slot_major", -1)
    sm = p["slot_major"] = int(P > 0 and dsm != 0 and (dsm > 0 or (R >= 768 * 1024 and R >= 6 * P)))
    bands = p["bands"] = counted_bands if counted_bands and R > 0 and not sm and banded_bytes <= two_pass_bytes else 0
    p["count_digits"] = int(bands == 0 and P > 0 and tb <= 16 and R > 0 and not counted(R))
    p["key_shift"], p["depth_lo_bits"] = (32 - tb, lo) if pt else (0, 0)
    p["sort_tiles"] = int(pt and R > 0)
    p["tile_sort_fused"] = int(p["sort_tiles"] and o("tile_sort_fused", 1) != 0)
    n = max(P, nt, min(R // 8, 0x3FFFFFFF) if sm else 0)
    p["dup_threads"] = -(-n // 256) * 256
    return p
