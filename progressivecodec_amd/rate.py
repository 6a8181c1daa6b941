"""Rate-controlled tiled coding (libpc_rate.so, rate_csrc/pc_rate.h): one 8-bit image in at most N bytes, every
tile at the level of the quality list that an allocator picks for it.

  tile_distortion        decoded tiles + the original image -> the exact integer weighted squared error per tile and channel, one
                         pass over the tiles on the GPU (no stitched image is needed)
  allocate               (bytes, distortion) per tile and level + a byte budget -> one level per tile; pure Python, exact integers
  encode_tiled_to_size   uint8 image -> (PCT2 container of at most target_bytes bytes, RatePlan)

The progressive codec makes the tables cheap: compress_levels codes every level of a batch of tiles with the base shared,
decompress_levels decodes them likewise, and a tile decodes to the same bits alone and in any batch, so the distortion measured at
encode time is the one the decoder gets.  The container is tiles.py's PCT2 (one level per tile); tiles.decode_tiled reads it.

Distortion.  A tile is judged by its OWN 8-bit rendering, e = Q(x_hat) - original with the stitch's quantiser Q, and a pixel counts
with the integer numerators ay * ax of the stitch's band weights over den = 2 * overlap (den = 1 without overlap): per image pixel
they sum to den^2 exactly, so sum_t D_t / den^2 is the squared error of the image where tiles do not overlap and bounds the blended
error from above where they do.

There is no CPU fallback: CPU tensors raise ValueError before any device call.  Out of scope: a target PSNR (the dual problem), rate
control inside compress_with_ac, REM models and WACNN, a level-major layout, untiled images.
"""
import collections
import ctypes as C
from fractions import Fraction

from . import _imagelib, _tilecodec
from ._lib import PC_OK
from .pixels import ROUNDINGS
from .tiles import HEADER_BYTES, TileGrid, _check_tiles, _fit_tiles, _linear_tiles, _view3, grid_of, pack_tiled  # noqa: F401

LIB_PATH = _imagelib.lib_path("rate")

#: every symbol rate_csrc/pc_rate.h declares
EXPORTS = ["pc_rate_workspace_size", "pc_rate_tile_sse_u8", "pc_rate_plan", "pc_rate_strerror", "pc_rate_last_hip_error"]

TABLE_ENTRY_BYTES = 16                    # a tile's (offset, length) in the PCT1 / PCT2 table


def _prototypes():
    i64, vp, ci = C.c_int64, C.c_void_p, C.c_int
    u8v = [vp, ci, i64, i64]                                        # a u8 view: pointer, layout, plane / row stride in bytes
    return {
        "pc_rate_workspace_size": (C.c_size_t, [ci, ci]),
        "pc_rate_tile_sse_u8": (None, [vp, i64, i64, i64] + [ci] * 7 + u8v + [vp, C.c_size_t, vp, vp]),
        "pc_rate_plan": (None, [vp, i64, i64, i64] + u8v + [C.POINTER(ci)]),
        "pc_rate_strerror": (C.c_char_p, [ci]),
    }


def lib():
    return _imagelib.load(LIB_PATH, _prototypes)


class RateError(_imagelib.ImageLibError):
    _lib, _prefix = staticmethod(lib), "pc_rate"


#: what encode_tiled_to_size decided: levels[t] (index into the quality list), rates[t][l] (bytes tile t costs at level l, its table
#: entry included), dists[t][l] (tile_distortion summed over the channels), den (the weights' denominator per axis), container_bytes
#: (the length of the container) and predicted (the sum of the chosen dists)
RatePlan = collections.namedtuple("RatePlan", "levels rates dists den container_bytes predicted")


def _tile_limit(T):
    if T > 2048:
        raise ValueError(f"tile must be at most 2048 for the distortion sums to fit 63 bits, got {T}")


def tile_distortion(x_hat_tiles, grid, ref, first_tile=0, ref_layout="hwc", rounding="nearest"):
    """x_hat_tiles: float32 cuda [n,3,T,T], the decoded tiles first_tile .. first_tile + n - 1 of grid's row-major ny x nx grid (a
    linear range, not a rectangle; grid's own rectangle is ignored; any tile / channel / row strides, unit stride along a row), ref: the
    original uint8 H x W image in ref_layout -> int64 cuda [n,3]: per tile and channel the sum over the tile's pixels inside the image
    of ay * ax * (Q(x_hat) - ref)^2, exact (pc_rate.h).  A tile's sums do not depend on which range it is part of."""
    import torch
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be 'nearest' or 'trunc', got {rounding!r}")
    g, n, x = _linear_tiles(grid, x_hat_tiles, first_tile, "image", _tile_limit)
    first_tile = int(first_tile)
    r4, rview, rhw = _view3(ref, ref_layout, "ref")
    if rhw != (g.H, g.W) or r4.device != x.device:
        raise ValueError(f"ref must be the {g.H}x{g.W} image on {x.device}, got {tuple(ref.shape)} on {ref.device}")
    if g.H == 1:                                                        # the stride of a one-row image is never used and may be anything
        rview = rview[:3] + (max(rview[3], g.W * (3 if ref_layout == "hwc" else 1)),)
    if x.device.type != "cuda":
        raise ValueError(f"x_hat_tiles must be on a GPU (there is no CPU fallback), got {x.device}")
    L = lib()
    with torch.cuda.device(x.device):
        nbytes = L.pc_rate_workspace_size(g.T, n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
        out = torch.empty((n, 3), dtype=torch.int64, device=x.device)
        rc = L.pc_rate_tile_sse_u8(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), g.H, g.W, g.T, g.O, first_tile, n,
                                   ROUNDINGS[rounding], *rview, ws.data_ptr(), nbytes, out.data_ptr(),
                                   torch.cuda.current_stream(x.device).cuda_stream)
    del r4
    if rc != PC_OK:
        raise RateError(rc, "pc_rate_tile_sse_u8")
    return out


def plan(x_hat_tiles, ref, ref_layout="hwc"):
    """pc_rate_plan for tensors (host only, nothing is launched or copied): True where tile_distortion of exactly these tensors takes
    the wide-access path.  ref is a 3-D uint8 tensor whose strides already fit a view."""
    x = x_hat_tiles
    view = (ref.data_ptr(), 0, 0, ref.stride(0)) if ref_layout == "hwc" else (ref.data_ptr(), 1, ref.stride(0), ref.stride(1))
    wide = C.c_int(-1)
    rc = lib().pc_rate_plan(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), *view, C.byref(wide))
    if rc != PC_OK:
        raise RateError(rc, "pc_rate_plan")
    return bool(wide.value)


# -- the allocator -------------------------------------------------------------------------------------------------------------------

def _hull(rate, dist):
    """The level indices of one tile on the lower convex hull of its (rate, distortion) points, by ascending rate."""
    n = len(rate)
    keep = [l for l in range(n)
            if not any(rate[m] <= rate[l] and dist[m] <= dist[l] and ((rate[m], dist[m]) != (rate[l], dist[l]) or m < l) for m in range(n))]
    keep.sort(key=lambda l: rate[l])                                    # rates are distinct now, distortion falls as rate rises
    hull = []
    for l in keep:
        while len(hull) >= 2:
            a, b = hull[-2], hull[-1]
            # b stays only if the step a -> b is strictly steeper than b -> l
            if (dist[a] - dist[b]) * (rate[l] - rate[b]) > (dist[b] - dist[l]) * (rate[b] - rate[a]):
                break
            hull.pop()
        hull.append(l)
    return hull


def allocate(rates, dists, budget, importance=None):
    """rates[t][l] (ints, bytes), dists[t][l] (ints), levels in the caller's order, neither assumed monotone; budget (int, bytes);
    importance[t] (positive numbers, taken exactly through Fraction) multiplies tile t's distortions -> the level index of every
    tile, total rate <= budget.  Exact integer / Fraction arithmetic throughout.

    1. per tile, levels that another level dominates (rate <= and distortion <=; of full ties the lower index stays) are dropped, and
       of the rest the lower convex hull is kept, by ascending rate;
    2. every tile starts at its cheapest hull point; ValueError (its message holds the minimum) if that exceeds the budget;
    3. hull steps are taken by -dD/dR, steepest first (compared by cross-multiplication, ties to the lower tile index); a step that
       fits is taken and the tile's next step becomes eligible, one that does not fit freezes its tile;
    4. if the best uniform level (the same index for every tile) that fits is strictly better than that, it is returned instead: the
       result is never worse than any uniform level that fits."""
    n = len(rates)
    if n < 1 or len(dists) != n:
        raise ValueError("rates and dists need one row per tile, at least one tile")
    nl = len(rates[0])
    if nl < 1 or any(len(r) != nl for r in rates) or any(len(d) != nl for d in dists):
        raise ValueError("every tile needs the same number of levels, at least one")
    for row in list(rates) + list(dists):
        if any(isinstance(v, bool) or not isinstance(v, int) for v in row):
            raise TypeError("rates and dists must be Python ints")
    if isinstance(budget, bool) or not isinstance(budget, int):
        raise TypeError("budget must be an int")
    if importance is None:
        imp = [Fraction(1)] * n
    else:
        imp = [Fraction(v) for v in importance]
        if len(imp) != n or any(v <= 0 for v in imp):
            raise ValueError("importance needs one positive number per tile")
    hulls = [_hull(rates[t], dists[t]) for t in range(n)]
    minimum = sum(rates[t][hulls[t][0]] for t in range(n))
    if minimum > budget:
        raise ValueError(f"the budget of {budget} bytes is below the minimum of {minimum} bytes (every tile at its cheapest level)")
    steps = []
    for t, h in enumerate(hulls):
        for k in range(1, len(h)):
            dr, dd = rates[t][h[k]] - rates[t][h[k - 1]], dists[t][h[k - 1]] - dists[t][h[k]]
            steps.append((-(imp[t] * dd) / dr, t, k))
    # a tile's steps fall strictly in steepness along its hull, so this one order is the order in which they become the steepest
    # eligible step; Fractions compare by cross-multiplication
    steps.sort()
    pos, frozen, left = [0] * n, [False] * n, budget - minimum
    for _, t, k in steps:
        if frozen[t]:
            continue
        dr = rates[t][hulls[t][k]] - rates[t][hulls[t][k - 1]]
        if dr <= left:
            left -= dr
            pos[t] = k
        else:
            frozen[t] = True
    levels = [hulls[t][pos[t]] for t in range(n)]
    total = sum(imp[t] * dists[t][levels[t]] for t in range(n))
    best = None
    for l in range(nl):
        if sum(rates[t][l] for t in range(n)) <= budget:
            d = sum(imp[t] * dists[t][l] for t in range(n))
            if best is None or d < best[0]:
                best = (d, l)
    if best is not None and best[0] < total:
        levels = [best[1]] * n
    return levels


# -- the encoder ---------------------------------------------------------------------------------------------------------------------

def encode_tiled_to_size(model, img, qualities, target_bytes, tile=512, overlap=0, mask_pol="point-based-std", layout="hwc",
                         rounding="nearest", importance=None, max_tiles_per_call=32):
    """uint8 cuda image [H,W,3] / [3,H,W] -> (PCT2 container of at most target_bytes bytes, RatePlan): every tile at the level of
    `qualities` that allocate() picks from the bytes each level costs (the tile's single-level PCB1 container plus its table entry)
    and the distortion it leaves (tile_distortion of the tile decoded at that level, judged as `rounding` will render it, summed over
    the channels), optionally weighted by importance ([ny][nx] or a flat list, one positive number per tile).  ValueError if even the
    cheapest level of every tile does not fit.  The tiles are cut, coded at every level (compress_levels), decoded again
    (decompress_levels) and measured max_tiles_per_call at a time, so a call holds at most max_tiles_per_call * (1 + len(qualities))
    tile tensors on the device; neither the bytes nor the plan depend on it."""
    import torch
    from . import tiles
    qualities = _tilecodec.levels_of(qualities)
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be 'nearest' or 'trunc', got {rounding!r}")
    step = _tilecodec.tiles_per_call(max_tiles_per_call)
    target_bytes = int(target_bytes)
    t4, view, (H, W) = _view3(img, layout, "img")
    g = grid_of(H, W, tile, overlap)
    n = g.ny * g.nx
    importance = _tilecodec.importance_of(importance, g)
    TL = tiles.lib()

    def cut(a, b):
        with torch.cuda.device(t4.device):
            x = torch.empty((b, 3, g.T, g.T), dtype=torch.float32, device=t4.device)
            k = 0
            for i, j, m in _tilecodec.row_pieces(a, b, g.nx):
                rc = TL.pc_tiles_cut_u8(*view, H, W, g.T, g.O, i, j, 1, m, x[k:].data_ptr(), torch.cuda.current_stream(t4.device).cuda_stream)
                if rc != PC_OK:
                    raise tiles.TilesError(rc, "pc_tiles_cut_u8")
                k += m
        return x

    def measure(a, b, decoded):
        d = torch.stack([tile_distortion(o["x_hat"], g, t4[0], a, layout, rounding).sum(1) for o in decoded], 1).tolist()   # [b][levels]
        return [[int(v) for v in row] for row in d]
    bufs, dists = _tilecodec.encode_items(model, n, step, qualities, mask_pol, g.T, cut, measure)
    del t4
    rates = [[TABLE_ENTRY_BYTES + len(p) for p in row] for row in bufs]
    levels = allocate(rates, dists, target_bytes - HEADER_BYTES, importance)
    buf = pack_tiled([bufs[t][levels[t]] for t in range(n)], g.H, g.W, g.T, g.O, per_tile_levels=True)
    return buf, RatePlan(levels, rates, dists, 2 * g.O if g.O else 1, len(buf), sum(dists[t][levels[t]] for t in range(n)))
