"""Float64 host reference of bnf_predictive_combinations (include/bnf.h): linear combinations of the rows of the sample
paths, from the per-row draws `predictive_samples` returns.

The bar of a cell follows from rounding alone.  Every product coef * x is rounded once (relative 2^-53), and summing the
n_k products of a form takes n_k - 1 additions in ANY order, each rounded once, none with a partial sum above
absum = sum |coef * x|: the computed value lies within (1 + (n_k - 1)) * 2^-53 * absum of the exact one to first order.
(n_k + 1) * 2^-52 * absum leaves a factor of two of margin and covers the second-order terms.  `math.fsum` of the float64
products is within one rounding of the exact sum of those products, which the + 1 pays for."""
import math

import numpy as np


def combine_ref(x, offsets, rows, coef):
  """x (S, R) the draws widened to float64, CSR over positions (offsets (K + 1,), rows (nnz,), coef (nnz,)) ->
  (value (S, K), absum (S, K)): per cell math.fsum of the float64 products coef[p] * x[s, rows[p]] and the sum of their
  absolute values.  A position whose row lies outside [0, R) adds nothing; an empty form is 0."""
  x = np.asarray(x, dtype=np.float64)
  offsets = np.asarray(offsets, dtype=np.int64)
  rows = np.asarray(rows, dtype=np.int64)
  coef = np.asarray(coef, dtype=np.float64)
  S, R = x.shape
  K = len(offsets) - 1
  value, absum = np.zeros((S, K)), np.zeros((S, K))
  inside = (rows >= 0) & (rows < R)
  for k in range(K):
    a, b = offsets[k], offsets[k + 1]
    keep = inside[a:b]
    if not keep.any():
      continue
    prod = x[:, rows[a:b][keep]] * coef[a:b][keep][None, :]
    absum[:, k] = np.abs(prod).sum(axis=1)
    value[:, k] = [math.fsum(prod[s]) for s in range(S)]
  return value, absum


def bar(offsets, absum):
  """The bar of every cell: (n_k + 1) * 2^-52 * absum, n_k the positions of form k."""
  n = np.diff(np.asarray(offsets, dtype=np.int64)).astype(np.float64)
  return (n[None, :] + 1.0) * 2.0 ** -52 * absum
