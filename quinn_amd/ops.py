"""The batched operator behind every solver: for B flat weight vectors at once, the MLP's
sum of squared errors over a (shared or per-member) set of data rows, its gradient, and
the predictions -- evaluated by the HIP kernels through the C ABI.

torch is used for device memory and streams only.
"""
import ctypes
import os
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from . import _lib
from ._lib import QuinnAmdError

_TORCH_DT = {"float64": torch.float64, "float32": torch.float32}
_QN_DT = {"float64": _lib.QN_F64, "float32": _lib.QN_F32}


def _ptr(t, rows=None):
    """Device address of the tensor t (of its rows `rows`, a slice); None for None."""
    if t is None:
        return None
    return (t if rows is None else t[rows]).data_ptr()


@dataclass(frozen=True)
class MLPArch:
    """dims = (d, h_1, ..., h_L, o); flat layout [W_0, b_0, W_1, b_1, ...] with W row-major
    (out x in), i.e. module.parameters() order (reference quinn/nns/nnwrap.py:70-77)."""
    dims: Tuple[int, ...]
    activ: str = "tanh"
    bias: bool = True

    @property
    def nparams(self):
        return sum(a * b + (b if self.bias else 0) for a, b in zip(self.dims[:-1], self.dims[1:]))

    @property
    def nweights(self):
        return sum(a * b for a, b in zip(self.dims[:-1], self.dims[1:]))

    def param_shapes(self):
        """Shapes of the module's parameter tensors in parameters() order."""
        shapes = []
        for a, b in zip(self.dims[:-1], self.dims[1:]):
            shapes.append((b, a))
            if self.bias:
                shapes.append((b,))
        return shapes

    def create_desc(self, L):
        dims = (ctypes.c_int * len(self.dims))(*self.dims)
        h = ctypes.c_void_p()
        _lib.check(L.qn_mlp_desc_create(dims, len(self.dims), _lib.ACT_CODES[self.activ], int(self.bias),
                                        ctypes.byref(h)), "qn_mlp_desc_create")
        return h

    def flops_fwd(self, n):
        """2*N*Wn."""
        return 2 * n * self.nweights

    def flops_fwdbwd(self, n):
        """6*N*Wn - 2*N*d*h_1 (no input gradient for the first layer)."""
        return 6 * n * self.nweights - 2 * n * self.dims[0] * self.dims[1]

    @staticmethod
    def from_module(nnmodel):
        """Pattern-match Sequential(Linear, act, Linear, ..., Linear) -- directly, or as the
        `.nnmodel` attribute of a quinn-style MLP (reference quinn/nns/mlp.py:86).  A quinn-style
        residual network (attributes of quinn/nns/rnet.py:16-127) yields an `RNetArch`."""
        if RNetArch.matches(nnmodel):
            return RNetArch.from_module(nnmodel)
        seq = nnmodel
        if isinstance(seq, torch.nn.Linear):                   # a bare linear model (reference examples/ex_lreg_mcmc.py:54)
            seq = torch.nn.Sequential(seq)
        if not isinstance(seq, torch.nn.Sequential):
            seq = getattr(nnmodel, "nnmodel", None)
        if not isinstance(seq, torch.nn.Sequential):
            raise NotImplementedError(
                f"{type(nnmodel).__name__}: only MLPs built as Sequential(Linear, act, ..., Linear) "
                "are handled by the MI355X path")
        mods = list(seq)
        dims, acts, bias = [], set(), None
        expect_linear = True
        for m in mods:
            if expect_linear:
                if not isinstance(m, torch.nn.Linear):
                    raise NotImplementedError(f"unexpected layer {type(m).__name__} (wanted Linear)")
                if not dims:
                    dims.append(m.in_features)
                elif dims[-1] != m.in_features:
                    raise ValueError("layer widths do not chain")
                dims.append(m.out_features)
                b = m.bias is not None
                if bias is None:
                    bias = b
                elif bias != b:
                    raise NotImplementedError("mixed bias / no-bias layers")
                expect_linear = False
            else:
                if isinstance(m, torch.nn.Tanh):
                    acts.add("tanh")
                elif isinstance(m, torch.nn.ReLU):
                    acts.add("relu")
                elif isinstance(m, torch.nn.Identity):
                    acts.add("identity")
                else:
                    raise NotImplementedError(f"activation {type(m).__name__} is not handled")
                expect_linear = True
        if expect_linear or len(dims) < 2:
            raise NotImplementedError("module must end with a Linear layer")
        if len(acts) > 1:
            raise NotImplementedError("mixed activations")
        return MLPArch(tuple(dims), acts.pop() if acts else "identity", bool(bias))


@dataclass(frozen=True)
class RNetArch:
    """Residual network of the reference (quinn/nns/rnet.py:16-165): optional pre layer (with
    activation), `nsteps = nlayers + 1` residual steps out += h * act(W_i out + b_i) (or plain
    layers if `mlp`), optional linear post layer.  `coef[i][k]` expresses the weight
    parameterisation W_i = sum_k coef[i][k] ww_k (rnet.py:217-380, all linear in the ww_k).
    Flat layout = parameters() order: weight_pre, bias_pre, weight_post, bias_post, ww_*, bb_*."""
    indim: int
    rdim: int
    outdim: int
    nsteps: int
    coef: Tuple[Tuple[float, ...], ...]
    activ: str = "tanh"
    bias: bool = True
    layer_pre: bool = False
    layer_post: bool = False
    mlp: bool = False
    uses: Tuple[Tuple[bool, ...], ...] = ()     # uses[i][k]: tensor k enters step i at all (default: every one does)

    @property
    def dims(self):
        return (self.indim, self.rdim, self.outdim)

    @property
    def npar(self):
        return len(self.coef[0])

    def param_shapes(self):
        r = self.rdim
        shapes = []
        if self.layer_pre:
            shapes += [(r, self.indim), (r,)]
        if self.layer_post:
            shapes += [(self.outdim, r), (self.outdim,)]
        shapes += [(r, r)] * self.npar
        if self.bias:
            shapes += [(r,)] * self.npar
        return shapes

    @property
    def nparams(self):
        return sum(int(np.prod(s)) for s in self.param_shapes())

    @property
    def nweights(self):
        """Multiply-accumulates per data row."""
        r = self.rdim
        return (r * self.indim if self.layer_pre else 0) + self.nsteps * r * r + \
            (self.outdim * r if self.layer_post else 0)

    def flops_fwd(self, n):
        return 2 * n * self.nweights

    def flops_fwdbwd(self, n):
        return 6 * n * self.nweights - (2 * n * self.rdim * self.indim if self.layer_pre else 0)

    def create_desc(self, L):
        if self.activ not in ("tanh", "identity"):
            raise NotImplementedError("RNet activations: tanh (nonlin=True) or identity")
        flat = [float(c) for row in self.coef for c in row]
        arr = (ctypes.c_double * len(flat))(*flat)
        h = ctypes.c_void_p()
        _lib.check(L.qn_rnet_desc_create(self.indim, self.rdim, self.outdim, self.nsteps, self.npar, arr,
                                         _lib.ACT_CODES[self.activ], int(self.bias), int(self.layer_pre),
                                         int(self.layer_post), int(self.mlp), ctypes.byref(h)),
                   "qn_rnet_desc_create")
        if self.uses:
            u = [1 if v else 0 for row in self.uses for v in row]
            _lib.check(L.qn_rnet_desc_set_uses(h, (ctypes.c_ubyte * len(u))(*u), len(u)), "qn_rnet_desc_set_uses")
        return h

    @staticmethod
    def matches(nnmodel):
        return all(hasattr(nnmodel, a) for a in ("rdim", "nlayers", "wp_function", "step_size", "layer_pre",
                                                 "layer_post", "biasorno", "mlp"))

    @staticmethod
    def from_module(nnmodel):
        """From this package's `RNet` or the reference's (same attributes).  The weight
        parameterisation is probed with unit 'parameters' to get its coefficients, and checked to
        be linear."""
        if getattr(nnmodel, "final_layer", None) is not None:
            raise NotImplementedError("RNet final_layer is outside the MI355X hot path")
        wp = nnmodel.wp_function
        npar, nsteps = int(wp.npar), int(nnmodel.nlayers) + 1
        coef, uses = [], []
        for i in range(nsteps):
            t = nnmodel.step_size * i                                  # rnet.py:146
            row = []
            # does tensor k enter the step at all?  A NaN there shows in the result if it does -- also through a zero
            # coefficient (the polynomials multiply t^k out; NonPar picks one tensor and never touches the others)
            uses.append(tuple(bool(np.isnan(float(wp([float('nan') if q == k else 0.0 for q in range(npar)], t)))) for k in range(npar)))
            for k in range(npar):
                e = [1.0 if q == k else 0.0 for q in range(npar)]
                c = float(wp(e, t))
                if float(wp([2.0 * v for v in e], t)) != 2.0 * c or float(wp([0.0] * npar, t)) != 0.0:
                    raise NotImplementedError("weight parameterisation must be linear in its parameters")
                row.append(c)
            coef.append(tuple(row))
        act = nnmodel.activ
        activ = "tanh" if isinstance(act, torch.nn.Tanh) else "identity" if isinstance(act, torch.nn.Identity) \
            else None
        if activ is None:
            raise NotImplementedError(f"RNet activation {type(act).__name__}")
        return RNetArch(int(nnmodel.indim), int(nnmodel.rdim), int(nnmodel.outdim), nsteps, tuple(coef), activ,
                        bool(nnmodel.biasorno), bool(nnmodel.layer_pre), bool(nnmodel.layer_post),
                        bool(nnmodel.mlp), tuple(uses))


def flatten_module(nnmodel):
    """Flat float64 numpy vector of module.parameters() (reference nnwrap.py:70-77)."""
    return np.concatenate([p.detach().cpu().double().flatten().numpy() for p in nnmodel.parameters()])


def default_device(device=None):
    if device is not None:
        dev = torch.device(device)
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if dev is None or dev.type != "cuda" or not torch.cuda.is_available():
        raise QuinnAmdError("quinn_amd needs an AMD GPU (HIP device) -- there is no CPU fallback")
    return dev


class BatchedMLP:
    """Device-resident dataset + architecture descriptor + workspace; calls the C ABI."""

    def __init__(self, arch: MLPArch, x, y, device=None, dtype="float64", max_workspace_bytes=48 << 30):
        self.arch = arch
        self.device = default_device(device)
        if dtype not in _TORCH_DT:
            raise ValueError(f"dtype {dtype!r}")
        self.dtype = dtype
        self.tdt = _TORCH_DT[dtype]
        self.qdt = _QN_DT[dtype]
        self.max_ws = int(max_workspace_bytes)
        self._L = _lib.lib()
        self._desc = h = arch.create_desc(self._L)
        self.p = int(self._L.qn_mlp_num_params(h))
        assert self.p == arch.nparams
        self._ws = None
        self.set_data(x, y)

    def __del__(self):
        try:
            if getattr(self, "_desc", None):
                self._L.qn_mlp_desc_destroy(self._desc)
                self._desc = None
        except Exception:
            pass

    # ------------------------------------------------------------------ data / buffers
    def _dev(self, a, dt=None):
        dt = dt or self.tdt
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dt).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), device=self.device).to(dt).contiguous()

    def set_data(self, x, y):
        d, o = self.arch.dims[0], self.arch.dims[-1]
        self.X = self._dev(x).reshape(-1, d)
        self.N = self.X.shape[0]
        if y is None:
            self.Y = torch.zeros(self.N, o, device=self.device, dtype=self.tdt)
        else:
            self.Y = self._dev(y).reshape(-1, o)
        if self.Y.shape[0] != self.N:
            raise ValueError("x and y row counts differ")
        self.G = None                                # gradient observations belong to the rows (set_grad_data)

    def workspace_bytes(self, B, Nb, want_grad):
        return int(self._L.qn_workspace_bytes(self._desc, B, Nb, int(want_grad), self.qdt))

    def path(self, B, Nb=None, want_grad=False):
        return int(self._L.qn_mlp_path(self._desc, B, Nb or self.N, int(want_grad), self.qdt))

    def arith(self, B, Nb=None, want_grad=False):
        """`_lib.ARITH_PLAIN` / `ARITH_I8_FUSED` / `ARITH_I8_WIDE` / `ARITH_I8_LAYERS`: the arithmetic the next call with these
        sizes forms the hidden-layer products in (qn_mlp_arith)."""
        return int(self._L.qn_mlp_arith(self._desc, B, Nb or self.N, int(want_grad), self.qdt))

    def set_path(self, path):
        """Force a kernel family for THIS operator (`_lib.PATH_AUTO` / `PATH_GENERIC` / `PATH_FUSED`; tests and
        profiling); returns the previous setting.  Per descriptor: other operators are unaffected."""
        return int(self._L.qn_mlp_desc_set_path(self._desc, int(path)))

    def set_plan_batch(self, batch):
        """Split every chain's rows as a launch of max(B, batch) chains would (qn_mlp_desc_set_plan_batch): a batch evaluated
        as several smaller launches then gives the one-launch results bit for bit.  Returns the previous setting."""
        return int(self._L.qn_mlp_desc_set_plan_batch(self._desc, int(batch)))

    def use_exact_float64(self):
        """Plain float64 arithmetic for THIS operator: under `PATH_AUTO` the float64 operator of 64 / 128 / 256-wide tanh
        networks runs the sliced int8-product kernels (operands rounded to 2^-47 of their row / activation scale: a
        norm-wise 47-bit bound, ~1e-14 .. 1e-13 on SSE / gradients of ordinary networks).  This selects the float64-MFMA
        fused kernels where the shape allows (`PATH_FUSED_DP`), the layer-wise float64 kernels otherwise (`PATH_GENERIC`).
        Returns the path taken."""
        from . import _lib as L
        self.set_path(L.PATH_FUSED_DP)
        try:
            ok = self.path(1, self.N, True) == L.PATH_FUSED and self.path(1, self.N, False) == L.PATH_FUSED
        except Exception:
            ok = False
        if not ok:
            self.set_path(L.PATH_GENERIC)
        return L.PATH_FUSED_DP if ok else L.PATH_GENERIC

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _fit_chunk(self, B, query, name, zero_ok=False):
        """(members per call, workspace bytes): min(B, 65535) members -- one per blockIdx.y / .z, the grid limit of the C
        ABI -- halved until `query(bc)` bytes fit `max_workspace_bytes`.  A 0-byte answer is the refusal of the query `name`
        unless `zero_ok`."""
        bc = min(B, 65535)
        while True:
            nbytes = int(query(bc))
            if nbytes == 0 and not zero_ok:
                raise QuinnAmdError(f"{name}: {self._L.qn_last_error().decode()}")
            if bc <= 1 or nbytes <= self.max_ws:
                return bc, nbytes
            bc = (bc + 1) // 2

    def _chunk(self, B, Nb, want_grad):
        return self._fit_chunk(B, lambda bc: self.workspace_bytes(bc, Nb, want_grad), "qn_workspace_bytes", zero_ok=True)[0]

    def _run_chunked(self, B, query, name, launch, zero_ok=False):
        """The member-chunked call of every operator: `launch(m, nb, tail)` -- one C call and its `_lib.check` -- for every
        slice m of nb members that `_fit_chunk` allows; `tail` = (workspace, its bytes, the current torch stream), the last
        three arguments of the C entry points."""
        bc, nbytes = self._fit_chunk(B, query, name, zero_ok)
        ws = self._workspace(nbytes)
        tail = (ws.data_ptr(), ws.numel(), _lib.stream(self.device))
        with torch.cuda.device(self.device):
            for b0 in range(0, B, bc):
                b1 = min(B, b0 + bc)
                launch(slice(b0, b1), b1 - b0, tail)

    def _row_idx(self, row_idx, B, N):
        """(int32 device tensor [B, Nb] or None, Nb): member b sees the rows row_idx[b]; all N without `row_idx`."""
        if row_idx is None:
            return None, N
        if not isinstance(row_idx, torch.Tensor):
            row_idx = np.asarray(row_idx)
        ridx = torch.as_tensor(row_idx, device=self.device).to(torch.int32).contiguous().reshape(B, -1)
        return ridx, ridx.shape[1]

    def _rows(self, x):
        """The stored X, or the query points x as a [N, d] device tensor."""
        return self.X if x is None else self._dev(x).reshape(-1, self.arch.dims[0])

    def weights(self, W):
        """[B, p] device tensor in the compute dtype (numpy float64 input is uploaded)."""
        Wt = self._dev(W)
        if Wt.dim() == 1:
            Wt = Wt.unsqueeze(0)
        if Wt.shape[1] != self.p:
            raise ValueError(f"weight vectors have {Wt.shape[1]} entries, the network has {self.p}")
        return Wt

    # ------------------------------------------------------------------ the operator
    def _call(self, W, row_idx, want_pred, want_grad, X=None, Y=None, out=None):
        X = self.X if X is None else X
        Y = self.Y if Y is None else Y
        N = X.shape[0]
        Wt = self.weights(W)
        B = Wt.shape[0]
        ridx, Nb = self._row_idx(row_idx, B, N)
        o = self.arch.dims[-1]
        if out is not None:                          # caller-owned result buffers (engines that run inside a HIP graph)
            sse, grad = out
            if sse.shape != (B,) or sse.dtype != torch.float64 or not sse.is_contiguous() or \
                    (want_grad and (grad.shape != (B, self.p) or grad.dtype != self.tdt or not grad.is_contiguous())):
                raise ValueError("out=(sse [B] float64, grad [B, p] compute dtype) does not match the call")
        else:
            sse = torch.empty(B, dtype=torch.float64, device=self.device)
            grad = torch.empty(B, self.p, dtype=self.tdt, device=self.device) if want_grad else None
        pred = torch.empty(B, Nb, o, dtype=self.tdt, device=self.device) if want_pred else None
        if B == 0:                                   # nothing to evaluate (e.g. an empty shard of chains)
            return sse, pred, grad
        fn, what = (self._L.qn_mlp_sse_fwdbwd, "qn_mlp_sse_fwdbwd") if want_grad else (self._L.qn_mlp_sse_fwd, "qn_mlp_sse_fwd")

        def launch(m, nb, tail):
            outs = [_ptr(sse, m), _ptr(pred, m)] + ([_ptr(grad, m)] if want_grad else [])
            _lib.check(fn(self._desc, self.qdt, _ptr(Wt, m), X.data_ptr(), Y.data_ptr(), _ptr(ridx, m), nb, N, Nb, *outs, *tail),
                       what)
        # a 0-byte workspace is an answer here (kernels that need none), not a refusal
        self._run_chunked(B, lambda bc: self.workspace_bytes(bc, Nb, want_grad), "qn_workspace_bytes", launch, zero_ok=True)
        return sse, pred, grad

    def sse(self, W, row_idx=None):
        """sum_{n,o} (y - f_W(x))^2 for every weight vector: float64 device tensor [B]."""
        return self._call(W, row_idx, False, False)[0]

    def sse_parts(self, W):
        """[B, parts] float64 partial sums whose left-to-right sum is `sse(W)` bit for bit (qn_mlp_sse_fwd_parts): the
        forward without its final summation launch, for `qn_mcmc_accept`, which adds the handful of numbers itself."""
        Wt = self.weights(W)
        B, N = Wt.shape[0], self.N
        if B == 0 or self._chunk(B, N, False) < B or os.environ.get("QUINN_AMD_NO_PARTS"):     # (env: A/B measurements)
            return self.sse(Wt).reshape(B, 1)
        parts = int(self._L.qn_mlp_sse_parts(self._desc, B, N, self.qdt))
        if parts < 1:
            raise _lib.QuinnAmdError("qn_mlp_sse_parts failed")
        out = torch.empty(B, parts, dtype=torch.float64, device=self.device)
        ws = self._workspace(self.workspace_bytes(B, N, False))
        with torch.cuda.device(self.device):
            _lib.check(self._L.qn_mlp_sse_fwd_parts(self._desc, self.qdt, Wt.data_ptr(), self.X.data_ptr(), self.Y.data_ptr(),
                                                    None, B, N, N, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    _lib.stream(self.device)), "qn_mlp_sse_fwd_parts")
        return out

    def sse_grad(self, W, row_idx=None, out=None):
        """(sse [B] float64, d sse / d W [B, p] compute dtype), device tensors; `out=(sse, grad)` writes into the
        caller's buffers instead of allocating."""
        s, _, g = self._call(W, row_idx, False, True, out=out)
        return s, g

    @staticmethod
    def _check_rows(what, W, name="W"):
        """W (or cur) of a fold / Gibbs round: a contiguous float64 device tensor [C, p]; returns (C, p)."""
        if not isinstance(W, torch.Tensor) or W.dtype != torch.float64 or W.dim() != 2 or not W.is_contiguous() or not W.is_cuda:
            raise ValueError(f"{what}: {name} is a contiguous float64 device tensor [C, p]")
        return W.shape

    @staticmethod
    def _check_fold(what, W, grad, sse, sse_stride):
        """The outputs of a fold at W [C, p] (checked by `_check_rows`): grad [C, p] float64 / float32 and sse (C * sse_stride
        float64), either None; returns the QN_* code of grad's dtype."""
        gdt = _lib.QN_F64
        if grad is not None:
            if grad.shape != W.shape or grad.dtype not in (torch.float64, torch.float32) or not grad.is_contiguous():
                raise ValueError(f"{what}: grad is a contiguous float64 / float32 tensor of W's shape")
            gdt = _lib.QN_F64 if grad.dtype == torch.float64 else _lib.QN_F32
        if sse is not None and (sse.dtype != torch.float64 or not sse.is_contiguous() or sse_stride < 1 or
                                sse.numel() != W.shape[0] * int(sse_stride)):
            raise ValueError(f"{what}: sse is a contiguous float64 tensor of C * sse_stride entries")
        return gdt

    def prior_fold(self, W, lam, c0, sse=None, grad=None, sse_stride=1):
        """Fold the Gaussian weight prior into the outputs of the forward / gradient call just made at W [C, p] float64
        (qn_prior_fold, one launch on the current stream, in place): grad [C, p] float64 / float32 += (2 lam) W,
        sse[c * sse_stride] += lam |W[c]|^2 + c0 (sse float64, [C] or [C, sse_stride]: column 0 receives the term).
        `quinn_amd.mcmc.prior.fold_constants` gives (lam, c0)."""
        C, p = self._check_rows("prior_fold", W)
        gdt = self._check_fold("prior_fold", W, grad, sse, sse_stride)
        if C == 0:
            return
        with torch.cuda.device(self.device):
            _lib.check(self._L.qn_prior_fold(W.data_ptr(), float(lam), float(c0), _ptr(grad), gdt, _ptr(sse), int(sse_stride),
                                             C, p, _lib.stream(self.device)), "qn_prior_fold")

    def _check_groups(self, what, lam, c0, seg, C, lead=()):
        """lam [*lead, C, G], c0 [*lead, C] float64 and seg [G + 1] int64, contiguous device tensors; returns G."""
        if not isinstance(seg, torch.Tensor) or seg.dtype != torch.int64 or seg.dim() != 1 or not seg.is_contiguous() or \
                not seg.is_cuda or not 2 <= seg.numel() <= 33:
            raise ValueError(f"{what}: seg is a contiguous int64 device tensor [G + 1], 1 <= G <= 32")
        G = seg.numel() - 1
        for t, shape, name in ((lam, lead + (C, G), "lam"), (c0, lead + (C,), "c0")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or \
                    not t.is_cuda:
                raise ValueError(f"{what}: {name} is a contiguous float64 device tensor {list(shape)}")
        return G

    def prior_fold_g(self, W, lam, c0, seg, sse=None, grad=None, sse_stride=1):
        """`prior_fold` with one precision per weight group and chain, read from device tensors (qn_prior_fold_g, one launch on
        the current stream, in place): grad [C, p] += (2 lam[c, g(j)]) W, sse[c * sse_stride] += sum_g lam[c, g] S_g + c0[c].
        lam [C, G], c0 [C] float64; seg [G + 1] int64, the group bounds (`quinn_amd.mcmc.hyper.fold_constants_g`,
        `group_segments`)."""
        C, p = self._check_rows("prior_fold_g", W)
        G = self._check_groups("prior_fold_g", lam, c0, seg, C)
        gdt = self._check_fold("prior_fold_g", W, grad, sse, sse_stride)
        if C == 0:
            return
        with torch.cuda.device(self.device):
            _lib.check(self._L.qn_prior_fold_g(W.data_ptr(), lam.data_ptr(), c0.data_ptr(), seg.data_ptr(), G, _ptr(grad), gdt,
                                               _ptr(sse), int(sse_stride), C, p, _lib.stream(self.device)), "qn_prior_fold_g")

    @staticmethod
    def _check_gibbs(what, cur, grad_cur, cur_lp, best_lp, lps, step):
        """The state a Gibbs round refreshes, cur [C, p] checked by `_check_rows`: grad_cur [C, p], cur_lp, best_lp [2, C], lps
        [C, nmcmc + 1] float64 and step [2] int64."""
        C, p = cur.shape
        for t, shape, name in ((grad_cur, (C, p), "grad_cur"), (cur_lp, (2, C), "cur_lp"), (best_lp, (2, C), "best_lp")):
            if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"{what}: {name} is a contiguous float64 device tensor {list(shape)}")
        if lps.dtype != torch.float64 or lps.dim() != 2 or lps.shape[0] != C or lps.shape[1] < 2 or not lps.is_contiguous():
            raise ValueError(f"{what}: lps is a contiguous float64 tensor [C, nmcmc + 1], nmcmc >= 1")
        if step.dtype != torch.int64 or step.numel() != 2 or not step.is_contiguous():
            raise ValueError(f"{what}: step is the double-buffered int64 step counter [2]")

    def hyper_gibbs(self, cur, grad_cur, cur_lp, best_lp, lps, lam, c0, seg, taus, step, sigma, a0, b0, round, chain0, seed,
                    parity, hyper_parity):
        """One Gibbs round of the group precisions after the step just decided (qn_hyper_gibbs, one launch on the current
        stream; `quinn_amd.mcmc.hyper.gibbs_round` restates it): cur, grad_cur [C, p], cur_lp, best_lp [2, C], lps
        [C, nmcmc + 1], lam [2, C, G], c0 [2, C] float64; seg [G + 1], step [2] int64; taus [C, nrounds + 1, G] float64 or
        None.  Slot `parity` of the scalars and slot `hyper_parity` of lam / c0 are read, the other slots written: the caller
        flips both."""
        C, p = self._check_rows("hyper_gibbs", cur, "cur")
        G = self._check_groups("hyper_gibbs", lam, c0, seg, C, lead=(2,))
        self._check_gibbs("hyper_gibbs", cur, grad_cur, cur_lp, best_lp, lps, step)
        nrounds = int(round) + 1
        if taus is not None:
            if taus.dtype != torch.float64 or taus.dim() != 3 or taus.shape[0] != C or taus.shape[2] != G or \
                    taus.shape[1] < 2 or not taus.is_contiguous():
                raise ValueError("hyper_gibbs: taus is a contiguous float64 tensor [C, nrounds + 1, G], nrounds >= 1")
            nrounds = taus.shape[1] - 1
        if C == 0:
            return
        with torch.cuda.device(self.device):
            _lib.check(self._L.qn_hyper_gibbs(cur.data_ptr(), grad_cur.data_ptr(), cur_lp.data_ptr(), best_lp.data_ptr(),
                                              lps.data_ptr(), lam.data_ptr(), c0.data_ptr(), seg.data_ptr(), _ptr(taus),
                                              step.data_ptr(), float(sigma), float(a0), float(b0), G, int(round), nrounds, C,
                                              int(chain0), p, lps.shape[1] - 1, int(seed), int(parity), int(hyper_parity),
                                              _lib.stream(self.device)), "qn_hyper_gibbs")

    def _check_noise(self, what, kappa, d0, lam, c0, seg, C, lead=()):
        """kappa, d0 [*lead, C] float64 contiguous device tensors; the weight prior lam [C, G], c0 [C], seg [G + 1] or three
        None (G = 0); returns G."""
        for t, name in ((kappa, "kappa"), (d0, "d0")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != lead + (C,) or \
                    not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"{what}: {name} is a contiguous float64 device tensor {list(lead + (C,))}")
        if lam is None and c0 is None and seg is None:
            return 0
        if lam is None or c0 is None or seg is None:
            raise ValueError(f"{what}: lam, c0 and seg go together (all None: no weight prior)")
        return self._check_groups(what, lam, c0, seg, C)

    def noise_fold(self, W, kappa, d0, lam=None, c0=None, seg=None, sse=None, grad=None, sse_stride=1):
        """Fold the per-chain noise level and the weight prior into the outputs of the gradient call just made at W [C, p]
        float64 (qn_noise_fold, ONE launch on the current stream, in place; `quinn_amd.mcmc.noise.fold_n` restates it):
        grad [C, p] <- kappa[c] grad + (2 lam[c, g(j)]) W, sse[c * sse_stride] <- (kappa[c] sse + sum_g lam[c, g] S_g + c0[c])
        + d0[c].  kappa, d0 [C] float64 (`noise.fold_constants_n`); lam [C, G], c0 [C], seg [G + 1] as in `prior_fold_g`, or
        all None: no weight prior."""
        C, p = self._check_rows("noise_fold", W)
        G = self._check_noise("noise_fold", kappa, d0, lam, c0, seg, C)
        gdt = self._check_fold("noise_fold", W, grad, sse, sse_stride)
        if C == 0:
            return
        with torch.cuda.device(self.device):
            _lib.check(self._L.qn_noise_fold(W.data_ptr(), kappa.data_ptr(), d0.data_ptr(), _ptr(lam), _ptr(c0), _ptr(seg), G,
                                             _ptr(grad), gdt, _ptr(sse), int(sse_stride), C, p, _lib.stream(self.device)),
                       "qn_noise_fold")

    def noise_gibbs(self, cur, grad_cur, cur_lp, best_lp, lps, kappa, d0, lam, c0, seg, sig, step, sigma, a0, b0, n, round,
                    chain0, seed, parity, noise_parity, sse_rec=None):
        """One Gibbs round of the noise level after the step just decided (qn_noise_gibbs, one launch on the current stream;
        `quinn_amd.mcmc.noise.gibbs_round` restates it): cur, grad_cur [C, p], cur_lp, best_lp, kappa, d0 [2, C], lps
        [C, nmcmc + 1] float64; lam [C, G], c0 [C], seg [G + 1]: the CURRENT slot of the weight prior, or all None; step [2]
        int64; sig [C, nrounds + 1] float64 or None; n = N * o entries of y.  Slot `parity` of the scalars and slot
        `noise_parity` of kappa / d0 are read, the other slots written: the caller flips both.  sse_rec [C] float64 or None
        receives the data SSE the round recovered (diagnostics; the engines pass None)."""
        C, p = self._check_rows("noise_gibbs", cur, "cur")
        G = self._check_noise("noise_gibbs", kappa, d0, lam, c0, seg, C, lead=(2,))
        self._check_gibbs("noise_gibbs", cur, grad_cur, cur_lp, best_lp, lps, step)
        nrounds = int(round) + 1
        if sig is not None:
            if sig.dtype != torch.float64 or sig.dim() != 2 or sig.shape[0] != C or sig.shape[1] < 2 or not sig.is_contiguous():
                raise ValueError("noise_gibbs: sig is a contiguous float64 tensor [C, nrounds + 1], nrounds >= 1")
            nrounds = sig.shape[1] - 1
        if sse_rec is not None and (sse_rec.dtype != torch.float64 or tuple(sse_rec.shape) != (C,) or not sse_rec.is_contiguous()
                                    or not sse_rec.is_cuda):
            raise ValueError("noise_gibbs: sse_rec is a contiguous float64 device tensor [C]")
        if C == 0:
            return
        with torch.cuda.device(self.device):
            _lib.check(self._L.qn_noise_gibbs(cur.data_ptr(), grad_cur.data_ptr(), cur_lp.data_ptr(), best_lp.data_ptr(),
                                              lps.data_ptr(), kappa.data_ptr(), d0.data_ptr(), _ptr(lam), _ptr(c0), _ptr(seg),
                                              _ptr(sig), _ptr(sse_rec), step.data_ptr(), float(sigma), float(a0), float(b0), self.N, int(n), G,
                                              int(round), nrounds, C, int(chain0), p, lps.shape[1] - 1, int(seed), int(parity),
                                              int(noise_parity), _lib.stream(self.device)), "qn_noise_gibbs")

    def sse_pred(self, W, row_idx=None):
        s, pr, _ = self._call(W, row_idx, True, False)
        return s, pr

    def predict(self, W, x=None):
        """f_W(x) for every weight vector: [B, N, o] device tensor (x defaults to the stored X)."""
        X = self._rows(x)
        Y = None if x is None else torch.zeros(X.shape[0], self.arch.dims[-1], device=self.device, dtype=self.tdt)
        return self._call(W, None, True, False, X=X, Y=Y)[1]

    # ------------------------------------------------------------------ curvature (Laplace approximation)
    def curvature(self, W, kind, row_idx=None):
        """Curvature of sum_n |f_W(x_n) - y_n|^2 / 2 for every weight vector, float64 device tensor (qn_mlp_curv):
        kind "full" -> [B, p, p] exact Hessian (symmetric bit for bit); "diag" -> [B, p] empirical-Fisher diagonal
        (1/Nb) sum_n (d/dW |r_n|^2 / 2)^2; "ggn" -> [B, p, p] generalised Gauss-Newton matrix sum_n sum_k J_nk^T J_nk
        (J_nk = d f_k(x_n) / dW; positive semi-definite, symmetric bit for bit); "ggn_diag" -> [B, p] its diagonal (a sum over
        the rows, not a mean).  `row_idx` [B, Nb]: member b sees rows row_idx[b] only.  All B members go in ONE call:
        qn_mlp_curv loops over them on the host and its workspace does not depend on B."""
        code = check_curvature_args(self.arch, self.dtype, kind)
        Wt = self.weights(W)
        B = Wt.shape[0]
        ridx, Nb = self._row_idx(row_idx, B, self.N)
        shape = (B, self.p, self.p) if code in (_lib.CURV_HESS_FULL, _lib.CURV_GGN_FULL) else (B, self.p)
        out = torch.empty(shape, dtype=torch.float64, device=self.device)
        if B == 0:
            return out
        nbytes = int(self._L.qn_curv_workspace_bytes(self._desc, code, B, Nb))
        if nbytes == 0:
            raise QuinnAmdError(f"qn_curv_workspace_bytes: {self._L.qn_last_error().decode()}")
        ws = self._workspace(nbytes)
        with torch.cuda.device(self.device):
            _lib.check(self._L.qn_mlp_curv(self._desc, code, Wt.data_ptr(), self.X.data_ptr(), self.Y.data_ptr(), _ptr(ridx), B,
                                           self.N, Nb, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream(self.device)),
                       "qn_mlp_curv")
        return out

    # ------------------------------------------------------------------ linearised predictive (qn_mlp_glm_predict)
    def glm_predict(self, W, Sigma, x=None):
        """Closed-form predictive of the Gaussian weight posteriors N(W[b], Sigma[b]) under the network linearised at W[b]:
        (mean [B, N, o] = f_{W[b]}(x_n), cov [B, N, o, o] = J_nk Sigma[b] J_nl^T), float64 device tensors.  Sigma [B, p, p]
        (symmetric) or [B, p] (a diagonal); x defaults to the stored X.  The Jacobian is never stored; B is chunked so the
        workspace stays under `max_workspace_bytes`; a member's result does not depend on the chunking."""
        check_curvature_args(self.arch, self.dtype, "ggn")
        Wt = self.weights(W)
        B = Wt.shape[0]
        Sg = self._dev(Sigma, torch.float64)
        if Sg.shape == (B, self.p, self.p):
            kind = _lib.GLM_COV_FULL
        elif Sg.shape == (B, self.p):
            kind = _lib.GLM_COV_DIAG
        else:
            raise ValueError(f"Sigma has shape {tuple(Sg.shape)}; expected ({B}, {self.p}, {self.p}) or ({B}, {self.p})")
        X = self._rows(x)
        N, o = X.shape[0], self.arch.dims[-1]
        mean = torch.empty(B, N, o, dtype=torch.float64, device=self.device)
        cov = torch.empty(B, N, o, o, dtype=torch.float64, device=self.device)
        if B == 0 or N == 0:
            return mean, cov

        def launch(m, nb, tail):
            _lib.check(self._L.qn_mlp_glm_predict(self._desc, kind, _ptr(Wt, m), X.data_ptr(), _ptr(Sg, m), nb, N,
                                                  _ptr(mean, m), _ptr(cov, m), *tail), "qn_mlp_glm_predict")
        self._run_chunked(B, lambda bc: self._L.qn_glm_workspace_bytes(self._desc, kind, bc, N), "qn_glm_workspace_bytes", launch)
        return mean, cov

    # ------------------------------------------------------------------ Kronecker-factored Gauss-Newton (qn_kron.hip)
    def kron_layout(self):
        """`KronLayout` of this network (qn_kron_layout; no device needed)."""
        check_kron_args(self.arch, self.dtype)
        if getattr(self, "_kron_lay", None) is None:
            self._kron_lay = kron_layout(self.arch, self._L, self._desc)
        return self._kron_lay

    def kron_factors(self, W, row_idx=None):
        """Kronecker factors of the Gauss-Newton matrix of every weight vector (qn_mlp_kron_factors): (A [B, lenA],
        S [B, lenS], layout), float64 device tensors; `layout.A(A, i)` / `layout.S(S, i)` are the views [B, e_i, e_i] /
        [B, h_{i+1}, h_{i+1}] of layer i.  A_i = sum_n ~in_i ~in_i^T and S_i = sum_n sum_k g^k_i g^k_i^T are SUMS over the member's
        rows (`row_idx` [B, Nb]: member b sees rows row_idx[b] only), symmetric bit for bit; the layer block of the
        Gauss-Newton matrix is approximated by (S_i (x) A_i) / Nb."""
        lay = self.kron_layout()
        Wt = self.weights(W)
        B = Wt.shape[0]
        ridx, Nb = self._row_idx(row_idx, B, self.N)
        A = torch.empty(B, lay.lenA, dtype=torch.float64, device=self.device)
        S = torch.empty(B, lay.lenS, dtype=torch.float64, device=self.device)
        if B == 0:
            return A, S, lay

        def launch(m, nb, tail):
            _lib.check(self._L.qn_mlp_kron_factors(self._desc, _ptr(Wt, m), self.X.data_ptr(), _ptr(ridx, m), nb, self.N, Nb,
                                                   _ptr(A, m), _ptr(S, m), *tail), "qn_mlp_kron_factors")
        self._run_chunked(B, lambda bc: self._L.qn_kron_workspace_bytes(self._desc, bc, Nb), "qn_kron_workspace_bytes", launch)
        return A, S, lay

    def kron_glm_predict(self, W, UA, US, Dinv, x=None):
        """`glm_predict` for the Kronecker-factored posterior (qn_mlp_kron_glm_predict): (mean [B, N, o], cov [B, N, o, o]),
        float64 device tensors.  UA [B, lenA], US [B, lenS]: the eigenvector matrices of the factors (eigenvectors in the
        columns, as `torch.linalg.eigh` returns them), packed like the factors; Dinv [B, p] in kron order: the posterior
        variance of the eigen-pair (a, c) of each layer.  No p x p array is formed; x defaults to the stored X."""
        lay = self.kron_layout()
        Wt = self.weights(W)
        B = Wt.shape[0]
        UA = _f64_rows(self._dev(UA, torch.float64), "UA", B, lay.lenA)
        US = _f64_rows(self._dev(US, torch.float64), "US", B, lay.lenS)
        Dinv = _f64_rows(self._dev(Dinv, torch.float64), "Dinv", B, self.p)
        X = self._rows(x)
        N, o = X.shape[0], self.arch.dims[-1]
        mean = torch.empty(B, N, o, dtype=torch.float64, device=self.device)
        cov = torch.empty(B, N, o, o, dtype=torch.float64, device=self.device)
        if B == 0 or N == 0:
            return mean, cov

        def launch(m, nb, tail):
            _lib.check(self._L.qn_mlp_kron_glm_predict(self._desc, _ptr(Wt, m), X.data_ptr(), _ptr(UA, m), _ptr(US, m),
                                                       _ptr(Dinv, m), nb, N, _ptr(mean, m), _ptr(cov, m), *tail),
                       "qn_mlp_kron_glm_predict")
        self._run_chunked(B, lambda bc: self._L.qn_kron_glm_workspace_bytes(self._desc, bc, N), "qn_kron_glm_workspace_bytes",
                          launch)
        return mean, cov

    # ------------------------------------------------------------------ input derivatives (qn_sobolev.hip)
    def input_jacobian(self, W, x=None, want_pred=False):
        """d f_k(x_n) / d x_j at every weight vector: float64 device tensor [B, N, o, d] (qn_mlp_input_jac); with
        `want_pred` the pair (jacobian, predictions [B, N, o]) from the same pass.  x defaults to the stored X.  B is chunked
        so the workspace stays under `max_workspace_bytes`; a member's result does not depend on the chunking."""
        check_sobolev_args(self.arch, self.dtype)
        Wt = self.weights(W)
        B = Wt.shape[0]
        d, o = self.arch.dims[0], self.arch.dims[-1]
        X = self._rows(x)
        N = X.shape[0]
        jac = torch.empty(B, N, o, d, dtype=torch.float64, device=self.device)
        pred = torch.empty(B, N, o, dtype=torch.float64, device=self.device) if want_pred else None

        def launch(m, nb, tail):
            _lib.check(self._L.qn_mlp_input_jac(self._desc, _ptr(Wt, m), X.data_ptr(), None, nb, N, N, _ptr(pred, m),
                                                _ptr(jac, m), *tail), "qn_mlp_input_jac")
        if B > 0 and N > 0:
            self._run_chunked(B, lambda bc: self._L.qn_sobolev_workspace_bytes(self._desc, bc, N, 0),
                              "qn_sobolev_workspace_bytes", launch)
        return (jac, pred) if want_pred else jac

    def set_grad_data(self, g):
        """Gradient observations d y_k / d x_j of the stored rows: (N, d) for one output, or (N, o, d)."""
        check_sobolev_args(self.arch, self.dtype)
        d, o = self.arch.dims[0], self.arch.dims[-1]
        G = self._dev(g, torch.float64)
        if G.numel() != self.N * o * d or G.shape[0] != self.N:
            raise ValueError(f"gradient data of shape {tuple(G.shape)}: expected ({self.N}, {o}, {d})"
                             + (f" or ({self.N}, {d})" if o == 1 else ""))
        self.G = G.reshape(self.N, o, d).contiguous()

    def sobolev(self, W, wv, wg, row_idx=None, want_grad=True):
        """(sse [B], gsse [B], grad [B, p] or None), float64 device tensors (qn_mlp_sobolev_fwdbwd):
        sse = sum_n |f - y|^2, gsse = sum_n sum_kj (d f_k / d x_j - G_kj)^2 over the rows (row_idx [B, Nb]: member b sees
        rows row_idx[b]), grad = wv d sse / dW + wg d gsse / dW.  Needs `set_grad_data`."""
        check_sobolev_args(self.arch, self.dtype)
        if getattr(self, "G", None) is None or self.G.shape[0] != self.N:
            raise ValueError("sobolev: no gradient observations for the stored rows; call set_grad_data(g) first")
        Wt = self.weights(W)
        B = Wt.shape[0]
        ridx, Nb = self._row_idx(row_idx, B, self.N)
        sse = torch.empty(B, dtype=torch.float64, device=self.device)
        gsse = torch.empty(B, dtype=torch.float64, device=self.device)
        grad = torch.empty(B, self.p, dtype=torch.float64, device=self.device) if want_grad else None
        if B == 0:
            return sse, gsse, grad

        def launch(m, nb, tail):
            _lib.check(self._L.qn_mlp_sobolev_fwdbwd(
                self._desc, _ptr(Wt, m), self.X.data_ptr(), self.Y.data_ptr(), self.G.data_ptr(), _ptr(ridx, m), nb, self.N,
                Nb, float(wv), float(wg), _ptr(sse, m), _ptr(gsse, m), _ptr(grad, m), *tail), "qn_mlp_sobolev_fwdbwd")
        self._run_chunked(B, lambda bc: self._L.qn_sobolev_workspace_bytes(self._desc, bc, Nb, int(want_grad)),
                          "qn_sobolev_workspace_bytes", launch)
        return sse, gsse, grad


SOBOLEV_MAX_D = SOBOLEV_MAX_O = 16


def _check_f64_mlp(arch, dtype, what, why=""):
    """The refusals every float64 extension operator shares: float32 (ValueError) and residual networks (NotImplementedError)."""
    if dtype != "float64":
        raise ValueError(f"{what}: the float64 operator is needed (got dtype {dtype!r}){why}")
    if not isinstance(arch, MLPArch):
        raise NotImplementedError(f"{what}: residual networks (RNet) are not supported; MLPs only")


def check_sobolev_args(arch, dtype):
    """Refuses what the input-derivative kernels (qn_mlp_input_jac / qn_mlp_sobolev_fwdbwd) do not take: float32 (they are
    float64 only), residual networks, more than 16 inputs or outputs."""
    _check_f64_mlp(arch, dtype, "input derivatives")
    if arch.dims[0] > SOBOLEV_MAX_D or arch.dims[-1] > SOBOLEV_MAX_O:
        raise NotImplementedError(f"input derivatives take d <= {SOBOLEV_MAX_D} inputs and o <= {SOBOLEV_MAX_O} outputs "
                                  f"(got d = {arch.dims[0]}, o = {arch.dims[-1]})")


def check_gradloss_args(arch, dtype, xtrn, gtrn, lam):
    """(N, o, d) float64 numpy gradient observations for `GradLoss` / loss_fn='gradloss'; refuses a missing or mis-shaped
    `gtrn`, a negative `lam` and what `check_sobolev_args` refuses."""
    check_sobolev_args(arch, dtype)
    if gtrn is None:
        raise ValueError("the gradient loss needs gtrn: the observed input gradients (N, d) or (N, o, d)")
    if lam is None or not np.isfinite(float(lam)) or float(lam) < 0.0:
        raise ValueError(f"the gradient loss needs a finite weight lam >= 0 (got {lam!r})")
    d, o = arch.dims[0], arch.dims[-1]
    n = np.asarray(xtrn).reshape(-1, d).shape[0]
    g = np.asarray(gtrn.detach().cpu() if isinstance(gtrn, torch.Tensor) else gtrn, dtype=np.float64)
    if g.shape not in ((n, o, d),) + (((n, d),) if o == 1 else ()):
        raise ValueError(f"gtrn has shape {g.shape}; expected ({n}, {o}, {d})" + (f" or ({n}, {d})" if o == 1 else ""))
    return g.reshape(n, o, d)


def check_curvature_args(arch, dtype, kind):
    """The `qn_mlp_curv` kind code for "full" / "diag" / "ggn" / "ggn_diag"; refuses what the curvature kernels do not take: float32 (the result
    is inverted, so it is float64 only), residual networks, other kinds."""
    codes = {"full": _lib.CURV_HESS_FULL, "diag": _lib.CURV_EF_DIAG, "ggn": _lib.CURV_GGN_FULL, "ggn_diag": _lib.CURV_GGN_DIAG}
    if kind not in codes:
        raise ValueError(f"curvature kind {kind!r}: 'full', 'diag', 'ggn' or 'ggn_diag'")
    _check_f64_mlp(arch, dtype, "curvature", ": the Hessian is inverted")
    return codes[kind]


def check_kron_args(arch, dtype):
    """Refuses what the Kronecker-factored kernels (qn_mlp_kron_factors / qn_mlp_kron_glm_predict / qn_kron_sample) do not take:
    float32 (the factors are eigendecomposed and inverted, so they are float64 only) and residual networks."""
    _check_f64_mlp(arch, dtype, "Kronecker-factored curvature", ": the factors are eigendecomposed and inverted")


@dataclass(frozen=True)
class KronLayout:
    """Where layer i sits in a member's packed Kronecker factors and in kron order (qn_kron_layout): A_i [e_i, e_i] at offA[i]
    of lenA doubles, S_i [h_{i+1}, h_{i+1}] at offS[i] of lenS, and (unit a, slot c) of a length-p vector at
    offK[i] + a e_i + c.  `perm` (numpy int64 [p]) maps kron order to flat order: flat = perm[kron]."""
    e: Tuple[int, ...]
    h: Tuple[int, ...]
    offA: Tuple[int, ...]
    offS: Tuple[int, ...]
    offK: Tuple[int, ...]
    lenA: int
    lenS: int
    p: int
    bias: bool

    def A(self, t, i):
        return t[..., self.offA[i]:self.offA[i] + self.e[i] ** 2].reshape(*t.shape[:-1], self.e[i], self.e[i])

    def S(self, t, i):
        return t[..., self.offS[i]:self.offS[i] + self.h[i] ** 2].reshape(*t.shape[:-1], self.h[i], self.h[i])

    def K(self, t, i):
        return t[..., self.offK[i]:self.offK[i] + self.h[i] * self.e[i]].reshape(*t.shape[:-1], self.h[i], self.e[i])

    @property
    def perm(self):
        out = np.empty(self.p, dtype=np.int64)
        for i, (e, h) in enumerate(zip(self.e, self.h)):
            d = e - 1 if self.bias else e                      # input slots that carry weights; slot d is the bias
            a, c = np.meshgrid(np.arange(h), np.arange(e), indexing="ij")
            flat = np.where(c < d, self.offK[i] + a * d + c, self.offK[i] + h * d + a)
            out[self.offK[i]:self.offK[i] + h * e] = flat.reshape(-1)
        return out


def kron_layout(arch, L=None, desc=None):
    """`KronLayout` of an MLPArch from qn_kron_layout (needs the built library, no device)."""
    L = L or _lib.lib()
    own = desc is None
    if own:
        desc = arch.create_desc(L)
    try:
        n = len(arch.dims) - 1
        arr = lambda: (ctypes.c_int64 * n)()                  # noqa: E731
        oa, os_, ok = arr(), arr(), arr()
        la, ls = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.qn_kron_layout(desc, oa, os_, ok, ctypes.byref(la), ctypes.byref(ls)), "qn_kron_layout")
    finally:
        if own:
            L.qn_mlp_desc_destroy(desc)
    hb = 1 if arch.bias else 0
    return KronLayout(tuple(d + hb for d in arch.dims[:-1]), tuple(arch.dims[1:]), tuple(oa), tuple(os_), tuple(ok),
                      int(la.value), int(ls.value), arch.nparams, bool(arch.bias))


def neg_log_post_from_sse(sse, n, sigma):
    """0.5*SSE/sigma^2 + (n/2)*log(2*pi) + n*log(sigma) in float64 with the operation order
    of the reference's NegLogPost.forward (quinn/nns/losses.py:198-200); sse: float64 array."""
    sse = np.asarray(sse, dtype=np.float64)
    sig = np.float64(sigma)
    val = 0.5 * sse / sig ** 2
    val = val + (n / 2) * np.log(2 * np.float64(np.pi))
    val = val + n * np.log(sig)
    return val


# ---------------------------------------------------------------------- SWAG (qn_swag_step / qn_swag_sample)
def check_swag_args(k, n_steps, c, cov_type):
    """True for the low-rank covariance, False for the diagonal one (any `cov_type` other than 'lowrank', as in the
    reference); refuses what NN_SWAG cannot form: k <= 1 (the draw divides by sqrt(k - 1)), c < 1, n_steps < 0 and, for
    'lowrank', fewer collections n_steps // c than the k deviation columns (the reference fails at prediction then)."""
    for name, v in (("k", k), ("n_steps", n_steps), ("c", c)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"SWAG {name} must be an integer (got {v!r})")
    if k <= 1:
        raise ValueError(f"SWAG k = {k}: need k > 1")
    if c < 1:
        raise ValueError(f"SWAG c = {c}: the collection period must be >= 1")
    if n_steps < 0:
        raise ValueError(f"SWAG n_steps = {n_steps}: need n_steps >= 0")
    lowrank = cov_type == "lowrank"
    if lowrank and n_steps // c < k:
        raise ValueError(f"SWAG cov_type 'lowrank' needs n_steps // c >= k: {n_steps} // {c} = {n_steps // c} "
                         f"collections for k = {k} deviation columns")
    return lowrank


def _f64_rows(t, name, B=None, p=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous float64 device tensor is needed")
    if B is not None and t.shape[0] != B or p is not None and t.shape[-1] != p:
        raise ValueError(f"{name}: shape {tuple(t.shape)} does not match B = {B}, p = {p}")
    return t


def _draw_members(js, B, dev):
    """(int32 device tensor [M], M) of the draws' member indices js (host or device ints), each checked on the host to lie in
    [0, B)."""
    js_h = np.asarray(js.cpu() if isinstance(js, torch.Tensor) else js).reshape(-1)
    if js_h.size and (js_h.min() < 0 or js_h.max() >= B):
        raise ValueError(f"member indices must lie in [0, {B})")
    return torch.as_tensor(js_h.astype(np.int32), device=dev), js_h.shape[0]


def swag_step(mode, W, G=None, lr=None, gscale=1.0, m1=None, m2=None, D=None, slot=0, n=0):
    """One `qn_swag_step` pass on the current torch stream.  W, m1, m2: [B, p] float64 device tensors (updated in place);
    G: [B, p] float64 or float32; lr: [B] float64; D: [B, K, p] float64 ring buffer or None.  mode: `_lib.SWAG_INIT`
    (m1 = W, m2 = W^2), `_lib.SWAG_SGD`, `_lib.SWAG_SGD_COLLECT` (SGD step, then the moments with count n and D[:, slot])."""
    B, p = _f64_rows(W, "W").shape
    for name, t in (("m1", m1), ("m2", m2)):
        if t is not None:
            _f64_rows(t, name, B, p)
    gdt = _lib.QN_F64
    if G is not None:
        if G.shape != (B, p) or G.dtype not in (torch.float64, torch.float32) or not G.is_contiguous():
            raise ValueError("G: a contiguous [B, p] float64 / float32 tensor is needed")
        gdt = _lib.QN_F64 if G.dtype == torch.float64 else _lib.QN_F32
    if lr is not None:
        _f64_rows(lr, "lr", B)
    K = 0
    if D is not None:
        _f64_rows(D, "D", B, p)
        K = D.shape[1]
    with torch.cuda.device(W.device):
        _lib.check(_lib.lib().qn_swag_step(int(mode), _ptr(W), _ptr(G), gdt, _ptr(lr), float(gscale), _ptr(m1), _ptr(m2), _ptr(D),
                                           K, int(slot), int(n), B, p, _lib.stream(W.device)), "qn_swag_step")


def swag_sample(mean, diag, D, js, z1, z2, drift, theta=None):
    """`qn_swag_sample` on the current torch stream: theta [M, p] float64 (device) of the M draws with member indices js
    (host or device ints, each in [0, B)), z1 [M, p], z2 [M, K] (ignored when D is None: diagonal covariance).
    drift=True moves mean[js[s]] to theta[s] in sample order, as the reference's predict_sample does."""
    B, p = _f64_rows(mean, "mean").shape
    _f64_rows(diag, "diag", B, p)
    dev = mean.device
    jsd, M = _draw_members(js, B, dev)
    if M == 0:
        return torch.empty(0, p, dtype=torch.float64, device=dev)
    z1d = _f64_rows(torch.as_tensor(z1, dtype=torch.float64, device=dev).reshape(M, p).contiguous(), "z1", M, p)
    K, z2d = 0, None
    if D is not None:
        _f64_rows(D, "D", B, p)
        K = D.shape[1]
        z2d = torch.as_tensor(z2, dtype=torch.float64, device=dev).reshape(M, K).contiguous()
    if theta is None:
        theta = torch.empty(M, p, dtype=torch.float64, device=dev)
    _f64_rows(theta, "theta", M, p)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().qn_swag_sample(mean.data_ptr(), diag.data_ptr(), _ptr(D), K, jsd.data_ptr(), z1d.data_ptr(),
                                             _ptr(z2d), M, B, p, int(bool(drift)), theta.data_ptr(), _lib.stream(dev)),
                   "qn_swag_sample")
    return theta


def kron_sample(arch, mean, UA, US, Dih, js, Z, out=None, op=None):
    """`qn_kron_sample` on the current torch stream: W [M, p] float64 (device, flat order) of the M draws of the
    Kronecker-factored posteriors: draw m uses member js[m] (host or device ints, each in [0, B)) and the standard normals
    Z[m] ([M, p], flat order); per layer W = mean + U_S (Z o Dih) U_A^T.  mean [B, p] flat; UA [B, lenA], US [B, lenS]
    eigenvector matrices packed like the factors; Dih [B, p] in kron order.  `op`: a float64 `BatchedMLP` of this architecture
    whose descriptor and layout are reused (callers that draw repeatedly); without it a descriptor is made for the call."""
    check_kron_args(arch, "float64")
    B, p = _f64_rows(mean, "mean").shape
    if p != arch.nparams:
        raise ValueError(f"mean has {p} columns, the network has {arch.nparams} parameters")
    dev = mean.device
    L = _lib.lib()
    if op is not None and (op.arch != arch or op.dtype != "float64"):
        raise ValueError("op: a float64 BatchedMLP of the same architecture is needed")
    desc = op._desc if op is not None else arch.create_desc(L)
    try:
        lay = op.kron_layout() if op is not None else kron_layout(arch, L, desc)
        _f64_rows(UA, "UA", B, lay.lenA)
        _f64_rows(US, "US", B, lay.lenS)
        _f64_rows(Dih, "Dih", B, p)
        jsd, M = _draw_members(js, B, dev)
        if M == 0:
            return torch.empty(0, p, dtype=torch.float64, device=dev)
        Zd = torch.as_tensor(Z, dtype=torch.float64, device=dev).reshape(M, p).contiguous()
        if out is None:
            out = torch.empty(M, p, dtype=torch.float64, device=dev)
        _f64_rows(out, "out", M, p)
        st = _lib.stream(dev)
        with torch.cuda.device(dev):
            for m0 in range(0, M, 65535):                         # draws, one per blockIdx.y: no workspace, nothing to fit
                m1 = min(M, m0 + 65535)
                _lib.check(L.qn_kron_sample(desc, mean.data_ptr(), UA.data_ptr(), US.data_ptr(), Dih.data_ptr(),
                                            jsd[m0:m1].data_ptr(), Zd[m0:m1].data_ptr(), out[m0:m1].data_ptr(), m1 - m0, st),
                           "qn_kron_sample")
    finally:
        if op is None:
            L.qn_mlp_desc_destroy(desc)
    return out
