"""What the tile and clip layers share on the host: the frame-parameter bytes of PCF1 / PCG1 / PCS1 / PCS2 and
of PCH1 / PCK1 / PCL1, the
tile table of PCT1 / PCT2 / PCS1 / PCS2 and the check of one of its entries, the encode loop, the decode loop and the argument
checks with fixed texts.  No library of its own and no device call: what needs a device -- the cut of a chunk of tiles, the
measurement of its decoded levels -- comes in as a callable, so everything here runs against a fake model on the host.

  frame_params      (fmt, matrix, range, upsample, bits) bytes -> names, or the container's refusal
  sited_head        the ten bytes of PCH1 / PCK1 / PCL1 (format as layout, shift, sx, sy; siting; matrix, range, upsample, bits)
  sited_params      those ten bytes -> names, or the container's refusal
  tile_table        header numbers -> (grid, [(offset, length)], payload start): geometry, "the whole table is there", the read
  entry_bytes       one table entry -> (the tile's PCB1 bytes, its parsed header), checked against buffer, tile size and contract
  encode_items      chunk, cut, compress_levels [, decompress_levels, measure], container.pack
  row_pieces        the cut walk of a linear tile range: one piece per grid row
  frame_pieces      the cut walk of a (frame, tile) work list: one piece per frame present
  level_strings     one level of one tile's PCB1 container; same_coding, one_level, check_contract: the refusals around it
  decode_positions  model.decompress per quality group and chunk, scattered to the tiles' places
"""
import ctypes as C
import struct

from ._lib import PC_OK
from .container import ContainerError


# -- containers ------------------------------------------------------------------------------------------------------------------------

def frame_params(f, m, r, u, bits, name):
    """the five frame-parameter bytes of the container `name` -> dict(fmt, matrix, range, upsample, bits)"""
    from .frames import FORMATS, RANGES, UPSAMPLES, _MATRIX_ID, _inv, bits_of
    fi, mi, ri, ui = _inv(FORMATS), _inv(_MATRIX_ID), _inv(RANGES), _inv(UPSAMPLES)
    if f not in fi or m not in mi or r not in ri or u not in ui:
        raise ContainerError(f"corrupt {name} header: fmt {f}, matrix {m}, range {r}, upsample {u}")
    if bits != bits_of(fi[f]):
        raise ContainerError(f"corrupt {name} header: {bits} bits for {fi[f]!r}")
    return {"fmt": fi[f], "matrix": mi[m], "range": ri[r], "upsample": ui[u], "bits": bits}


def sited_head(fmt, matrix, range, upsample, siting):
    """the ten frame-parameter bytes of PCH1 / PCK1 / PCL1: layout, shift, sx, sy, horizontal siting, vertical siting, matrix, range,
    upsample, bits"""
    from .chroma import FORMATS, SITINGS, _MATRIX_ID
    from .frames import RANGES, UPSAMPLES
    f, (hs, vs) = FORMATS[fmt], SITINGS[siting]
    return f.layout, f.shift, f.sx, f.sy, hs, vs, _MATRIX_ID[matrix], RANGES[range], UPSAMPLES[upsample], f.bits


def sited_params(lay, sh, sx, sy, hs, vs, m, r, u, bits, name):
    """sited_head's ten bytes, read from the container `name` -> dict(fmt, siting, matrix, range, upsample, bits)"""
    from .chroma import FORMATS, SITINGS, _MATRIX_ID, _inv
    from .frames import RANGES, UPSAMPLES
    fi, si, mi, ri, ui = _inv(FORMATS), _inv(SITINGS), _inv(_MATRIX_ID), _inv(RANGES), _inv(UPSAMPLES)
    if bits not in (8, 10):
        raise ContainerError(f"corrupt {name} header: {bits} bits")
    if (lay, bits, sh, sx, sy) not in fi or (hs, vs) not in si or m not in mi or r not in ri or u not in ui:
        raise ContainerError(f"corrupt {name} header: layout {lay}, shift {sh} at {bits} bits, subsampling {sx}x{sy}, siting {hs}, {vs}, "
                             f"matrix {m}, range {r}, upsample {u}")
    return {"fmt": fi[(lay, bits, sh, sx, sy)], "siting": si[(hs, vs)], "matrix": mi[m], "range": ri[r], "upsample": ui[u], "bits": bits}


def tile_table(buf, at, H, W, T, O, ny, nx, frames=1, head="header", what="image", table="tile table"):
    """The table of `frames` x ny x nx entries (offset u64, length u64) at byte `at` of buf -> (TileGrid (whole grid), the entries in
    stored order, the payload's start), after checking the geometry against pc_tiles_grid and grid_of and that the whole table is
    there.  head, what and table are the words of the refusals."""
    from . import tiles
    cy, cx = C.c_int(0), C.c_int(0)
    if max(H, W, T, O) >= 1 << 31 or tiles.lib().pc_tiles_grid(H, W, T, O, C.byref(cy), C.byref(cx)) != PC_OK:
        raise ContainerError(f"corrupt {head}: {what} {H}x{W}, tile {T}, overlap {O}")
    if (cy.value, cx.value) != (ny, nx):
        raise ContainerError(f"corrupt {head}: grid {ny}x{nx}, but a {H}x{W} {what} in tiles of {T} with overlap {O} has {cy.value}x{cx.value}")
    g = tiles.grid_of(H, W, T, O)
    if (g.ny, g.nx) != (ny, nx):
        raise ContainerError(f"corrupt {head}: grid")
    if frames < 1:
        raise ContainerError(f"corrupt {head}: no frames")
    start = at + 16 * frames * ny * nx
    if len(buf) < start:
        raise ContainerError(f"truncated {table}")
    flat = struct.unpack_from(f"<{2 * frames * ny * nx}Q", buf, at)
    return g, list(zip(flat[0::2], flat[1::2])), start


def entry_bytes(buf, hd, entry, where, owner="container"):
    """The PCB1 container a table entry = (offset, length) of the parsed header hd points at, and its parsed header, after checking
    the entry against the buffer, the PCB1 header against the tile size and its contract against hd's.  where ("tile 3") opens
    the refusals, owner names what hd was parsed from."""
    from . import container
    off, n = entry
    if off < hd["payload_start"] or off + n > len(buf):
        raise ContainerError(f"{where}: table entry ({off}, {n}) points outside the {len(buf)} bytes at hand (truncated or corrupt)")
    tb = bytes(buf[off:off + n])
    th = container.parse_header(tb)
    T = hd["grid"].T
    if th["image_size"] != (T, T) or tuple(th["shape"]) != (T // 64, T // 64):
        raise ContainerError(f"{where}: its container holds a {th['image_size'][0]}x{th['image_size'][1]} image, not a {T}x{T} tile")
    if th["contract"] != hd["contract"]:
        raise ContainerError(f"{where}: numeric contract 0x{th['contract']:08x}, the {owner}'s is 0x{hd['contract']:08x}")
    return tb, th


def check_contract(contract):
    from . import container
    if contract != container.build_contract_id():
        raise ContainerError(f"container was coded under numeric contract 0x{contract:08x}, this decoder implements "
                             f"0x{container.build_contract_id():08x}: the streams are not interchangeable (DESIGN.md section 2)")


# -- the encode loop -------------------------------------------------------------------------------------------------------------------

def encode_items(model, n, step, qualities, mask_pol, T, cut, measure=None):
    """The n work items (tiles of T x T) coded `step` at a time: cut(a, b) -> float32 [b,3,T,T] for the items a .. a + b - 1, one
    model.compress_levels per chunk, container.pack per item -> one multi-level PCB1 container per item.  With measure, the chunk
    is decoded again (model.decompress_levels) and measure(a, b, decoded) -- decoded[l]["x_hat"] the chunk's tiles at level l; it
    returns one entry per item and is done with the tiles when it returns -- is called once per chunk -> (bufs[item][level], each
    a single-level PCB1 container, what measure returned, item by item).  A chunk holds at most step * (1 + levels) tile tensors."""
    from . import container
    bufs, measured = [], []
    for a in range(0, n, step):
        b = min(step, n - a)
        x = cut(a, b)
        datas = model.compress_levels(x, qualities, mask_pol=mask_pol)
        del x
        strings = [d["strings"] for d in datas]
        shape = datas[0]["shape"]
        if measure is None:
            bufs += [container.pack(strings, shape, qualities, image_size=(T, T), mask_pol=mask_pol, image_index=m) for m in range(b)]
            continue
        decoded = model.decompress_levels(strings, shape, qualities, mask_pol)
        measured += measure(a, b, decoded)
        del decoded
        bufs += [[container.pack([strings[l]], shape, [q], image_size=(T, T), mask_pol=mask_pol, image_index=m) for l, q in enumerate(qualities)]
                 for m in range(b)]
    return bufs if measure is None else (bufs, measured)


def row_pieces(a, b, nx):
    """the tiles a .. a + b - 1 of a row-major grid nx wide, one piece per grid row -> (row, first column, count), in order"""
    k = 0
    while k < b:
        i, j = divmod(a + k, nx)
        m = min(b - k, nx - j)
        yield i, j, m
        k += m


def frame_pieces(chunk):
    """a chunk of (frame, tile) pairs in (frame, tile) order, one piece per frame present -> (frame, m0, m1): chunk[m0:m1]"""
    m0 = 0
    while m0 < len(chunk):
        m1 = m0
        while m1 < len(chunk) and chunk[m1][0] == chunk[m0][0]:
            m1 += 1
        yield chunk[m0][0], m0, m1
        m0 = m1


# -- the decode loop -------------------------------------------------------------------------------------------------------------------

def one_level(level, name):
    """the level argument for a container whose tiles hold one level each"""
    try:
        lv = int(level)
    except (TypeError, ValueError):
        lv = None
    if lv not in (-1, 0):
        raise ContainerError(f"a {name} container holds one level per tile: level must be -1 or 0, got {level!r}")


def level_strings(tb, th, level, where=""):
    """one level (index into the quality list, negative from the end) of one tile's PCB1 container -> (latent shape, quality, mask
    policy, strings); its contract is the caller's to check, once"""
    from . import container
    nl = len(th["qualities"])
    lv = int(level) + nl if int(level) < 0 else int(level)
    if not 0 <= lv < nl:
        raise ContainerError(f"{where}no level {level} among {nl}")
    strings, shape, qs, _, mask_pol = container.unpack(tb, levels=[lv], expect_contract=False)
    return tuple(shape), qs[0], mask_pol, strings[0]


def same_coding(key, first_key, where, first):
    """what the tiles of one decode must share: `where` was coded as key, the tile called `first` as first_key"""
    if key != first_key:
        raise ContainerError(f"{where} was coded as {key}, {first} as {first_key}")


def decode_positions(model, strings_of, groups, shape, mask_pol, step, n, prev=None):
    """The decoded tiles of n positions, float32 [n,3,T,T].  strings_of[p]: the strings of position p; groups: [(quality,
    [positions])], decoded in this order, step positions at a time (one model.decompress each) and placed at their positions;
    (shape, mask_pol): what all of them share.  Positions no group names keep prev's tiles (the previous frame's tensor, which is
    left as it is: the result is a clone).  A call that covers every position gives the model's tensor itself, no group at all
    gives prev itself."""
    import torch
    if not groups:
        return prev
    x_hat = None if sum(len(idx) for _, idx in groups) == n else prev.clone()
    for q, idx in groups:
        for a in range(0, len(idx), step):
            part = idx[a:a + step]
            chunk = [strings_of[p] for p in part]
            ys = [[s[0][i][0] for s in chunk] for i in range(len(chunk[0][0]))]                    # y_strings[slice][image]
            zs = [s[1][0] for s in chunk]
            dec = model.decompress([ys, zs], shape, q, mask_pol)["x_hat"]
            if len(part) == n:
                return dec
            if x_hat is None:
                x_hat = torch.empty((n,) + tuple(dec.shape[1:]), dtype=dec.dtype, device=dec.device)
            x_hat[torch.tensor(part, device=dec.device)] = dec
    return x_hat


# -- argument checks ---------------------------------------------------------------------------------------------------------------------

def max_tile(fmt):
    """the largest tile whose distortion sums fit 63 bits: T^4 (2^n - 1)^2 < 2^60; 1024 for the 10-bit formats of chroma.FORMATS"""
    from .chroma import FORMATS
    return 1024 if fmt in FORMATS and FORMATS[fmt].bits == 10 else 2048


def tile_limit(T, fmt):
    if T > max_tile(fmt):
        raise ValueError(f"tile must be at most {max_tile(fmt)} for the distortion sums of {fmt!r} to fit 63 bits, got {T}")


def tiles_per_call(max_tiles_per_call):
    step = int(max_tiles_per_call)
    if step < 1:
        raise ValueError(f"max_tiles_per_call must be at least 1, got {max_tiles_per_call}")
    return step


def levels_of(qualities):
    qualities = [float(q) for q in qualities]
    if not qualities:
        raise ValueError("at least one level")
    return qualities


def plane_weights_of(plane_weights):
    pw = list(plane_weights)
    if len(pw) != 3 or any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in pw) or not any(pw):
        raise ValueError(f"plane_weights must be three non-negative ints, not all zero, got {plane_weights!r}")
    return pw


def importance_of(importance, g):
    """importance ([ny][nx] or flat, or None) -> flat, one number per tile of g's whole grid"""
    if importance is None:
        return None
    importance = list(importance)
    if importance and isinstance(importance[0], (list, tuple)):
        importance = [v for row in importance for v in row]
    if len(importance) != g.ny * g.nx:
        raise ValueError(f"importance needs one number per tile of the {g.ny}x{g.nx} grid, got {len(importance)}")
    return importance


def frame_weights_of(frame_weights, F):
    if frame_weights is None:
        return None
    frame_weights = list(frame_weights)
    if len(frame_weights) != F:
        raise ValueError(f"frame_weights needs one number per frame of the clip, {F} in all, got {len(frame_weights)}")
    return frame_weights
