"""Host model of the conjugate gradients across ranks (amg_dist_pcg_*): the
rank-ordered dot product.

Test infrastructure only.  Every rank sums its own rows with the bits of
amg_vec_dot on its local length (pcg_ref.dev_dot) and the rank values are added
in rank order from 0.0, as the finish kernels of csrc/amg_pcg.hip add the
all-gathered slots.  pcg_ref.pcg_model with dot = dist_dot(row_starts) then has
the bits of the distributed recurrence.
"""
import pcg_ref


def dist_dot(row_starts):
    """dot(x, y) of the row partition row_starts (nranks + 1 first rows, level 0)"""
    rs = [int(a) for a in row_starts]

    def dot(x, y):
        s = 0.0
        for a, b in zip(rs[:-1], rs[1:]):
            s += pcg_ref.dev_dot(x[a:b], y[a:b])
        return s

    return dot


def dist_model(oracle, host, opts, f, iters, row_starts, x0=None):
    return pcg_ref.pcg_model(oracle, host, opts, f, iters, dist_dot(row_starts), x0)
