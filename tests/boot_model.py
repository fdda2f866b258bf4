"""The model of ss_reads_resample that the bootstrap tests hold the device to.

A record's weight is a pure function of (its bytes, seed, replicate): the second half of its digest (ss_flat_record_keys, host code)
goes through one splitmix64 round together with the seed and the replicate, and the top 32 bits are looked up in the cumulative
Poisson(1) table.  Everything here is numpy on uint64 (wrapping arithmetic) or `decimal`; nothing needs a device.
"""
import decimal

import numpy as np

M64 = (1 << 64) - 1


def poisson1_table():
    """T_k = floor(2^32 * e^-1 * sum_{i <= k} 1/i!), k = 0..12, with 80-digit decimals."""
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        e_inv = decimal.Decimal(-1).exp()
        out, acc, fact = [], decimal.Decimal(0), decimal.Decimal(1)
        for k in range(13):
            if k:
                fact *= k
            acc += decimal.Decimal(1) / fact
            out.append(int((decimal.Decimal(1 << 32) * e_inv * acc).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    return out


TABLE = np.array(poisson1_table(), np.uint64)


def weights_of_keys(key, seed, replicate):
    """key: np.uint64[n], the second digest half of every record -> np.int64[n] weights in 0..13."""
    mix = (0x9E3779B97F4A7C15 * (int(replicate) + 1) + 0xD6E8FEB86659FD93 * int(seed)) & M64
    with np.errstate(over="ignore"):
        x = np.asarray(key, np.uint64) + np.uint64(mix)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    u = x >> np.uint64(32)
    return (TABLE[None, :] <= u[:, None]).sum(axis=1).astype(np.int64)


def records_of(flat):
    return [p for p in bytes(flat).split(b"\n") if p]


def weights(L, flat, seed, replicate):
    """(records, weights) of a flat block: `L` is strainscan_amd._lib (ss_flat_record_keys runs on the host)."""
    recs = records_of(flat)
    if not recs:
        return recs, np.zeros(0, np.int64)
    keys = L.flat_record_keys(b"\n".join(recs) + b"\n")
    assert keys.shape == (len(recs), 2)
    return recs, weights_of_keys(keys[:, 1], seed, replicate)


def resampled(L, flat, seed, replicate):
    """The sorted records of the resampled set: every record of `flat` as often as its weight says."""
    recs, w = weights(L, flat, seed, replicate)
    return sorted(r for r, n in zip(recs, w.tolist()) for _ in range(n))
