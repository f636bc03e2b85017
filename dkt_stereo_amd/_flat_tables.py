"""The device table behind a kernel that walks a list of tensors as one flat range (csrc/flat_walk.h: dkt_ema_update,
dkt_adamw_step): one row of addresses per tensor list, then the exclusive prefix offsets of the sizes and their total."""
import torch

_TABLES = {}
_CAP = 16


def flat_tables(dev, *lists):
    """(table, row pointers, total) for equal-length lists of tensors on `dev`; sizes are those of the first list.
    ``ptrs[i]`` addresses the row of ``lists[i]``, ``ptrs[len(lists)]`` the count + 1 offsets.  Cached per set of addresses
    (the oldest of 16 entries goes first; the 16 are shared by every caller, the EMA and the optimizer tables together); a
    miss is staged through pinned memory and copied without blocking, so it does not synchronise."""
    sizes = tuple(t.numel() for t in lists[0])
    key = (dev,) + tuple(tuple(t.data_ptr() for t in ts) for ts in lists) + (sizes,)
    hit = _TABLES.get(key)
    if hit is None:
        off = [0]
        for n in sizes:
            off.append(off[-1] + n)
        rows = [[t.data_ptr() for t in ts] for ts in lists] + [off[:-1]]
        host = torch.tensor(rows, dtype=torch.int64).reshape(-1)
        host = torch.cat([host, torch.tensor([off[-1]], dtype=torch.int64)]).pin_memory()
        table = host.to(dev, non_blocking=True)
        n = len(sizes)
        hit = (table, [table[i * n:].data_ptr() for i in range(len(lists) + 1)], off[-1])
        if len(_TABLES) >= _CAP:
            _TABLES.pop(next(iter(_TABLES)))
        _TABLES[key] = hit
    return hit
