"""float64 NumPy restatement of the reference's ViewEmbeddingMLP (networks/embedding.py:35-62), forward and backward, and the accessors of
golden G40 (tools/gen_golden.py G40_view_embed_mlp).  The module's input is a function of the image id, so everything is stated on the
TABLE: row i = the module's value for image i; the per-ray form is a gather of its rows and the backward of a gather is the per-image sum
of the rows' gradients."""
import numpy as np

G40_CASES = ("shipped", "skip", "odd", "one", "wide")


def depth(p):
    return len([k for k in p if k.startswith("view_embed_linears.") and k.endswith(".weight")])


def param_keys(D):
    return ("img_embed",) + tuple(f"view_embed_linears.{i}.{w}" for i in range(D) for w in ("weight", "bias"))


def forward(p, skips, keep=None):
    """p: the reference's parameter names -> arrays -> feature table [n_img, W] (float64).  keep: a list that receives (input, output) of
    every layer"""
    e = np.asarray(p["img_embed"], np.float64)                                         # embedding.py:31-32,52: one row per image
    h = e                                                                              # :55
    for i in range(depth(p)):                                                          # :56
        w, b = (np.asarray(p[f"view_embed_linears.{i}.{s}"], np.float64) for s in ("weight", "bias"))
        x = h
        h = np.maximum(x @ w.T + b, 0.0)                                               # :57-58
        if keep is not None:
            keep.append((x, h))
        if i in skips:
            h = np.concatenate([e, h], -1)                                             # :59-60: the embedding columns come first
    return h                                                                           # :61-62


def backward(p, skips, d_table):
    """d_table [n_img, W]: what arrives at the feature table -> {parameter name: gradient} (float64)"""
    D, keep = depth(p), []
    forward(p, skips, keep)
    E = np.asarray(p["img_embed"]).shape[1]
    g = {"img_embed": np.zeros(np.asarray(p["img_embed"]).shape, np.float64)}
    d = np.asarray(d_table, np.float64)
    for i in reversed(range(D)):
        if i in skips:                                                                 # :60 backwards: the first E columns belong to the embedding row
            g["img_embed"] += d[:, :E]
            d = d[:, E:]
        x, h = keep[i]
        dpre = d * (h > 0)                                                             # :58
        w = np.asarray(p[f"view_embed_linears.{i}.weight"], np.float64)
        g[f"view_embed_linears.{i}.weight"] = dpre.T @ x                               # :57
        g[f"view_embed_linears.{i}.bias"] = dpre.sum(0)
        d = dpre @ w
    g["img_embed"] += d                                                                # :54-55: layer 0 reads the embedding row
    return g


def d_table_of_rows(n_img, ids, d_rows):
    """the gather's backward: per-image sums of the rows' gradients"""
    out = np.zeros((n_img, d_rows.shape[1]), np.float64)
    np.add.at(out, np.asarray(ids).reshape(-1), np.asarray(d_rows, np.float64))
    return out


def run(p, skips, ids, proj):
    """float64 table, rows = table[ids] and the gradients of sum(rows * proj)"""
    table = forward(p, skips)
    ids = np.asarray(ids).reshape(-1)
    return dict(table=table, out=table[ids], grads=backward(p, skips, d_table_of_rows(table.shape[0], ids, proj)))


def fence_margin(p, skips):
    """-> (smallest |pre| / (sum |w||x| + |b|) over every unit of every layer and image, the threshold 2 D (K + 1) 2^-24 of the layer where
    the ratio of the two is smallest): a float32 evaluation cannot flip a ReLU whose margin exceeds its threshold"""
    D, keep, worst = depth(p), [], (np.inf, 1.0)
    forward(p, skips, keep)
    for i, (x, _) in enumerate(keep):
        w, b = (np.asarray(p[f"view_embed_linears.{i}.{s}"], np.float64) for s in ("weight", "bias"))
        margin = float((np.abs(x @ w.T + b) / (np.abs(x) @ np.abs(w).T + np.abs(b))).min())
        thr = 2.0 * D * (w.shape[1] + 1) * 2.0 ** -24
        if margin / thr < worst[0] / worst[1]:
            worst = (margin, thr)
    return worst


def floor(p):
    """the a-priori float32 error of the computation itself: D (K_max + 1) 2^-24, K_max the longest dot product"""
    D = depth(p)
    return D * (max(np.asarray(p[f"view_embed_linears.{i}.weight"]).shape[1] for i in range(D)) + 1) * 2.0 ** -24


def g40_case(g, tag):
    """one case of golden G40 -> dict(D, W, E, n_img, skips, absent (image id or None), params, ids [R], proj [R, W], and per part
    ('alone', 'rigid', 'dsk') a dict of sd / cfg / inputs / proj / out / out64 / g / g64 / err_out / err_g)"""
    pre = tag + "."
    pick = lambda sub: {k[len(pre + sub):]: g[k] for k in g if k.startswith(pre + sub)}
    D, W, E, n_img, absent = (int(v) for v in g[pre + "cfg"])
    c = dict(D=D, W=W, E=E, n_img=n_img, absent=None if absent < 0 else absent, skips=[int(s) for s in g[pre + "skips"]], params=pick("sd."),
             ids=g[pre + "ids"].reshape(-1), proj=g[pre + "alone.proj"])
    for part in ("alone", "rigid", "dsk"):
        c[part] = dict(sd=pick(part + ".sd."), cfg=pick(part + ".cfg."), inputs=pick(part + ".in."), proj=pick(part + ".proj."), out=pick(part + ".out."), out64=pick(part + ".out64."),
                       g=pick(part + ".g."), g64=pick(part + ".g64."), err_out={k: float(v) for k, v in pick(part + ".ref_f32_err.out.").items()},
                       err_g={k: float(v) for k, v in pick(part + ".ref_f32_err.g.").items()})
    return c


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb else float(np.linalg.norm(a - b))
