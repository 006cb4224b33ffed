"""Molecules instead of atoms: the plan ``ta_compound`` reduces a staged slab of atoms by.

The electrolyte analyses (Fong, Bergstrom, McCloskey, Persson) are defined on the centre of mass of every molecule or ion, in
the barycentric frame of the system.  The frames are staged as atoms (``ta_stage_frame`` and ``unwrap=True`` need atoms); one
pass on the device (``k_compound`` behind ``ta_compound`` of ``include/ta_hip.h``) then replaces the slab by the slab of the
compounds' weighted centres, and every evaluation runs on it unchanged.
"""
from __future__ import annotations

import numpy as np

#: compound="..." -> the per-atom attribute of the group that labels it (MDAnalysis' names)
COMPOUND_ATTRS = {"residues": "resindices", "segments": "segindices", "molecules": "molnums", "fragments": "fragindices"}


def compound_plan(labels, per_atom_weights):
    """(ids, offsets, members, weights) for ``Context.compound``: ``ids`` the distinct labels in ``np.unique`` order,
    compound c = the member entries [offsets[c], offsets[c + 1]) of ``members`` (the atoms with label ids[c], in input
    order), ``weights`` the atoms' ``per_atom_weights`` in member order, normalised to sum to 1 within each compound.
    A compound whose weights sum to 0 raises ValueError."""
    labels = np.asarray(labels).ravel()
    w = np.asarray(per_atom_weights, dtype=np.float64).ravel()
    if w.size != labels.size:
        raise ValueError(f"compound_weights: {w.size} values for {labels.size} atoms")
    ids, index = np.unique(labels, return_inverse=True)
    index = np.asarray(index).ravel()
    members = np.argsort(index, kind="stable").astype(np.int32)
    counts = np.bincount(index, minlength=ids.size)
    offsets = np.zeros(ids.size + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    total = np.bincount(index, weights=w, minlength=ids.size)
    if np.any(total == 0) or not np.all(np.isfinite(total)):
        bad = ids[np.flatnonzero((total == 0) | ~np.isfinite(total))[0]]
        raise ValueError(f"compound {bad!r}: its weights sum to {total[ids == bad][0]}, so it has no weighted centre")
    weights = w[members] / total[index[members]]
    return ids, offsets, members, weights


def same_order(index, n_compounds):
    """every compound is one atom and the compounds come in the atoms' order: per atom and per compound are one thing"""
    return index.size == n_compounds and bool(np.array_equal(index, np.arange(n_compounds)))


def per_compound(values, index, n_compounds, name, per_atom=None):
    """One value per compound from ``values`` given per compound (returned as they are) or per atom (they must then be the
    same within every compound, else ValueError); ``index`` the compound of every atom.  ``per_atom``: True when the
    caller knows the values are per atom (a topology attribute), None: told apart by their number -- and when there are
    as many compounds as atoms in ANOTHER order (one-atom compounds, unsorted labels) that is a ValueError: the values
    would land on the wrong particles whichever way they were read."""
    a = np.asarray(values).ravel()
    if per_atom is None and a.size == n_compounds == index.size and not same_order(index, n_compounds):
        raise ValueError(f"{name}: {a.size} values for {index.size} atoms in {n_compounds} one-atom compounds whose order "
                         "(np.unique of the labels) is not the atoms': per atom or per compound cannot be told apart; "
                         "give the compound labels in increasing order")
    if a.size == n_compounds and not per_atom:
        return a
    if a.size != index.size:
        raise ValueError(f"{name}: {a.size} values for {n_compounds} compounds ({index.size} atoms)")
    first = np.full(n_compounds, -1, dtype=np.int64)
    first[index[::-1]] = np.arange(index.size - 1, -1, -1)  # the first atom of every compound
    out = a[first]
    if np.any(a != out[index]):
        n = int(np.flatnonzero(a != out[index])[0])
        raise ValueError(f"{name}: given per atom, it must be the same for all atoms of a compound; atom {n} has {a[n]!r}, "
                         f"the first atom of its compound {out[index[n]]!r}")
    return out
