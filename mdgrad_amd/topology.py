"""Topology helpers with the reference's names (torchmd/topology.py).  The neighbour search
runs in the HIP builders (csrc/nbr.hip); results come back in the reference's format.  The angle list
(generate_angle_list) is built from sorted index tensors on the list's own device, without the reference's
[M, M] mask over all directed pairs."""
import itertools

import torch

from . import _lib, ops


def compute_dis(xyz, nbr_list, offsets, cell):
    """torchmd/topology.py:5-12 (torch ops on the device; the pair kernels fuse this)."""
    nbr_list = nbr_list.to(xyz.device)
    cell = torch.diag(cell) if cell.dim() == 1 else cell
    return (xyz[nbr_list[:, 0]] - xyz[nbr_list[:, 1]] - offsets.matmul(cell)).pow(2).sum(1).sqrt()[:, None]


def generate_pair_index(N, index_tuple):
    """torchmd/topology.py:15-27."""
    mask_sel = torch.zeros(N, N)
    if index_tuple is not None:
        pair_mask = torch.LongTensor([list(items) for items in itertools.product(index_tuple[0], index_tuple[1])])
        mask_sel[pair_mask[:, 0], pair_mask[:, 1]] = 1
        mask_sel[pair_mask[:, 1], pair_mask[:, 0]] = 1
    return mask_sel


def generate_nbr_list(xyz, cutoff, cell, index_tuple=None, ex_pairs=None, get_dis=False):
    """torchmd/topology.py:30-73: minimum-image half list (i<j, lexicographic; a leading frame
    column for batched input) and image offsets.  xyz must be a HIP tensor."""
    _lib.require_gpu(xyz, "xyz")
    cs = _lib.make_cell(cell)
    N = xyz.shape[-2]
    mask = ops.build_mask(N, index_tuple, ex_pairs, xyz.device)
    frames = xyz.reshape(-1, N, 3)
    cellm = torch.as_tensor(cell, dtype=torch.float32, device=xyz.device)
    cellm = torch.diag(cellm) if cellm.dim() == 1 else cellm
    F = frames.shape[0]
    # all frames in ONE list build: the frames are groups of one stacked system (pairs never cross groups), so the
    # half list comes out sorted by (frame, i, j) -- the reference's order -- with one host sync for the pair count
    ell = ops.build_ell(frames.reshape(F * N, 3), cs, cutoff, mask, group=N if F > 1 else None)
    nbr, off = ell.half_list()
    if get_dis:
        flat = frames.reshape(F * N, 3)
        dis = compute_dis(flat, nbr, off, cellm).reshape(-1)
    if xyz.dim() > 2:
        frame = torch.div(nbr[:, :1], N, rounding_mode="floor")
        nbr = torch.cat([frame, nbr - frame * N], 1)
    if get_dis:
        return nbr, dis, off
    return nbr, off


def get_offsets(vecs, cell, device):
    """torchmd/topology.py:75-80 (non-strict >= on the + side, unlike generate_nbr_list)."""
    return -vecs.ge(0.5 * cell).to(torch.float).to(device) + vecs.lt(-0.5 * cell).to(torch.float).to(device)


def make_directed(nbr_list):
    """torchmd/topology.py:101-122: the list followed by the same rows with the two atom columns swapped."""
    return torch.cat([nbr_list, nbr_list[:, [0, 2, 1]]], 0)


ANGLE_LIST_MAX = 2 ** 31     # entries (rows x 4) beyond which generate_angle_list refuses


def generate_angle_list(nbr_list):
    """torchmd/topology.py:83-98: rows (frame, i, j, k) for every directed row (frame, i, j) of make_directed(nbr_list),
    in that row order, followed by its thirds k: the third atoms of the directed rows (frame, j, k), k != i, in directed-row
    order.  Same rows in the same order as the reference, from a stable sort of the directed rows by (frame, first atom)
    instead of the reference's [M, M] mask; runs on the list's device.  Raises ValueError when the list would exceed
    ANGLE_LIST_MAX entries or does not fit in memory."""
    assert nbr_list.shape[1] == 3
    d = make_directed(nbr_list.to(torch.long))
    M, dev = d.shape[0], d.device
    if M == 0:
        return torch.zeros(0, 4, dtype=torch.long, device=dev)
    span = int(d[:, 1:].max()) + 1
    key = d[:, 0] * span + d[:, 1]                          # group of directed rows that leave atom d[:, 1] of frame d[:, 0]
    order = torch.sort(key, stable=True)[1]                 # stable: each group keeps the directed-row order
    skey = key[order]
    want = d[:, 0] * span + d[:, 2]                         # row (f, i, j) takes the group of (f, j)
    lo = torch.searchsorted(skey, want)
    n = torch.searchsorted(skey, want, right=True) - lo
    total = int(n.sum())
    if 4 * total > ANGLE_LIST_MAX:
        raise ValueError("generate_angle_list: %d candidate triplets exceed the list limit of %d entries; "
                         "use angle_distribution(..., keep_angles=False) for the histogram alone" % (total, ANGLE_LIST_MAX))
    try:
        row = torch.repeat_interleave(torch.arange(M, device=dev), n)
        start = torch.cumsum(n, 0) - n
        cand = order[lo[row] + torch.arange(total, device=dev) - start[row]]
        third = d[cand, 2]
        keep = third != d[row, 1]
        return torch.cat([d[row[keep]], third[keep, None]], 1)
    except torch.cuda.OutOfMemoryError as e:
        raise ValueError("generate_angle_list: the triplet list does not fit in device memory (%s); "
                         "use angle_distribution(..., keep_angles=False) for the histogram alone" % e) from None


def chain_dihedrals(n_atoms, start=0):
    """[n_atoms - 3, 4] rows (i, i + 1, i + 2, i + 3) of a linear chain whose first atom is `start` (the quadruples the
    polymer demo's internal coordinates run over, demo/fold.py:57-72); empty below four atoms."""
    i = torch.arange(max(int(n_atoms) - 3, 0), dtype=torch.long)[:, None] + int(start)
    return i + torch.arange(4, dtype=torch.long)[None, :]


def dihedrals_from_bonds(bonds):
    """Every proper torsion (i, j, k, l) of a bond graph: i-j, j-k and k-l bonded, i != k, j != l, i != l (three-rings give
    none).  Each torsion appears once, with j < k, ordered lexicographically by (j, k, i, l).  bonds: [n_bonds, 2]; returns
    int64 [n, 4] on the host."""
    b = torch.as_tensor(bonds).detach().cpu().to(torch.long).reshape(-1, 2).tolist()
    nbrs = {}
    for i, j in b:
        if i != j:
            nbrs.setdefault(i, set()).add(j)
            nbrs.setdefault(j, set()).add(i)
    rows = []
    for j, k in sorted({(min(i, j), max(i, j)) for i, j in b if i != j}):
        for i in sorted(nbrs[j] - {k}):
            for l in sorted(nbrs[k] - {j, i}):
                rows.append((i, j, k, l))
    return torch.tensor(rows, dtype=torch.long).reshape(-1, 4)


def exclusions_from_bonds(bonds, n_bonds=2, return_separation=False):
    """Every pair i < j of a bond graph joined by a path of at most `n_bonds` bonds (n_bonds = 2: the 1-2 and 1-3 pairs a
    force field excludes from its non-bonded sums; 3 adds the 1-4 pairs), sorted and unique: int64 [P, 2] on the host.
    return_separation: also the length of the shortest such path per pair, int64 [P] -- so that a caller can scale the pairs
    three bonds apart (EwaldExclusions(..., scale=0.5 where it is 3)).  bonds: [n, 2]; self-bonds are ignored."""
    n_bonds = int(n_bonds)
    if n_bonds < 1:
        raise ValueError("exclusions_from_bonds: n_bonds must be at least 1 (got %d)" % n_bonds)
    nbrs = {}
    for i, j in torch.as_tensor(bonds).detach().cpu().to(torch.long).reshape(-1, 2).tolist():
        if i != j:
            nbrs.setdefault(i, set()).add(j)
            nbrs.setdefault(j, set()).add(i)
    sep = {}
    for a in sorted(nbrs):                                       # breadth-first from every atom, n_bonds levels deep
        seen, front = {a}, {a}
        for depth in range(1, n_bonds + 1):
            front = {c for b in front for c in nbrs[b]} - seen
            seen |= front
            for c in front:
                if a < c:
                    sep[(a, c)] = depth
    keys = sorted(sep)
    pairs = torch.tensor(keys, dtype=torch.long).reshape(-1, 2)
    if return_separation:
        return pairs, torch.tensor([sep[k] for k in keys], dtype=torch.long)
    return pairs
