"""Model-level API: ``quantize``, ``freeze``, ``requantize``, ``quantization_map`` (optimum/quanto/quantize.py:24-149)."""
from fnmatch import fnmatch
from typing import Any, Dict, List, Optional, Union

import torch

from .nn import QConv2d, QLayerNorm, QLinear, QModuleMixin, quantize_module
from .tensor import Optimizer, QTensor, WeightQBitsTensor, WeightQBytesTensor, qint2, qint4, qtype
from .tensor.weights import _fusable, conv2d_a8_scales_underflow

__all__ = ["quantize", "freeze", "requantize", "quantization_map", "fuse_output_quantization"]


def _set_module_by_name(parent: torch.nn.Module, name: str, child: torch.nn.Module) -> None:
    *path, leaf = name.split(".")
    for part in path:
        parent = getattr(parent, part)
    setattr(parent, leaf, child)


def _quantize_submodule(model, name, module, weights=None, activations=None, optimizer=None, layernorm=False):
    if layernorm and isinstance(module, torch.nn.LayerNorm) and not isinstance(module, QModuleMixin):
        # opt-in: QLayerNorm is not in the table of counterparts, which decides what the default quantize() does (None without an activation qtype)
        qmodule = QLayerNorm.from_module(module, weights=weights, activations=activations, optimizer=optimizer)
    else:
        qmodule = quantize_module(module, weights=weights, activations=activations, optimizer=optimizer)
    if qmodule is None:
        return False
    _set_module_by_name(model, name, qmodule)
    qmodule.name = name
    for pname, param in module.named_parameters():
        # the quantized module aliases the parameters: release the originals
        setattr(module, pname, None)
        del param
    return True


def _as_patterns(p: Optional[Union[str, List[str]]]):
    return [p] if isinstance(p, str) else p


def quantize(model: torch.nn.Module, weights: Optional[Union[str, qtype]] = None,
             activations: Optional[Union[str, qtype]] = None, optimizer: Optional[Optimizer] = None,
             include: Optional[Union[str, List[str]]] = None, exclude: Optional[Union[str, List[str]]] = None, layernorm: bool = False):
    """Replace every eligible submodule in place by its quantized counterpart.

    ``include`` / ``exclude`` are Unix shell-style patterns on module names (quantize.py:55-98).  Weights stay
    float (dynamically quantized in forward) until ``freeze``.

    ``layernorm=True`` (opt-in) also replaces every ``torch.nn.LayerNorm`` that passes include / exclude by a ``QLayerNorm`` when an
    activation qtype is given (the reference does so always, nn/qlayernorm.py): its output is then quantized at its ``output_scale``,
    which lets the Linears it feeds run on the stored codes.  The default leaves LayerNorms as float modules.
    """
    include, exclude = _as_patterns(include), _as_patterns(exclude)
    for name, module in list(model.named_modules()):
        if include is not None and not any(fnmatch(name, pattern) for pattern in include):
            continue
        if exclude is not None and any(fnmatch(name, pattern) for pattern in exclude):
            continue
        _quantize_submodule(model, name, module, weights=weights, activations=activations, optimizer=optimizer, layernorm=layernorm)


def requantize(model: torch.nn.Module, state_dict: Dict[str, Any], quantization_map: Dict[str, Dict[str, str]],
               device: torch.device = None, layernorm: bool = False):
    """Rebuild a frozen model from a flattened state dict + ``quantization_map`` (quantize.py:101-140).

    ``layernorm=True`` (opt-in): a ``torch.nn.LayerNorm`` the map names is rebuilt as a ``QLayerNorm`` and gets its input / output scales back
    (a checkpoint of ``quantize(..., layernorm=True)``, or one written by the reference); with the default it stays a float module and the
    warning below says so.

    One deliberate divergence from the reference: when the checkpoint's float dtype differs from the dtype ``model`` was built in
    (an fp32 checkpoint opened as a bf16 skeleton), the reference keeps the deserialized scale / shift as they are
    (nn/qmodule.py:161-207) and the module then mixes dtypes (its ``forward`` raises on fp32 scale x bf16 bias).  Here the rebuilt
    weight's scale and float shift are cast to the model's dtype - integers untouched - and a ``UserWarning`` names the modules:
    the dequantized weights are then the checkpoint's values re-rounded to the model dtype, not bit-identical to what was saved.
    Build the skeleton in the checkpoint's dtype to get the reference's bits."""
    if device is None:
        first = next(model.parameters(), None)  # (None: a model of LayerNorms without elementwise affine has no parameter)
        device = torch.device("cpu") if first is None or first.device.type == "meta" else first.device
    not_rebuilt = []
    for name, module in list(model.named_modules()):
        qconfig = quantization_map.get(name)
        if qconfig is None:
            continue
        weights = None if qconfig["weights"] == "none" else qconfig["weights"]
        activations = None if qconfig["activations"] == "none" else qconfig["activations"]
        if not _quantize_submodule(model, name, module, weights=weights, activations=activations, layernorm=layernorm):
            not_rebuilt.append(f"{name} ({type(module).__name__})")
    missing = sorted(set(quantization_map) - {n for n, _ in model.named_modules()})
    # Materialise what is still on the meta device, then load.  The float ``weight`` of a module whose quantized weight is in the
    # state dict is never materialised (the reference stages everything on the CPU, quantize.py:123-137; on the device that would
    # cost the full float model next to the quantized one): it stays on meta until ``load_state_dict(assign=True)`` replaces it.
    def serialized(prefix: str) -> bool:
        return any(k.startswith(prefix + "weight._") for k in state_dict)

    for name, m in model.named_modules():
        def move(t):
            if t.device.type == "meta":
                return torch.empty_like(t, device=device)
            return t.to(device)

        skip_weight = isinstance(m, QModuleMixin) and serialized(name + "." if name else "")
        for pname, p in list(m.named_parameters(recurse=False)):
            if skip_weight and pname == "weight" and p.device.type == "meta":
                continue
            setattr(m, pname, torch.nn.Parameter(move(p), requires_grad=p.requires_grad))
        for bname, b in list(m.named_buffers(recurse=False)):
            setattr(m, bname, move(b))
    # dtype of the model's own (non-quantized) parameters wins over the checkpoint's, as with a copying load_state_dict
    want = {k: v.dtype for k, v in list(model.named_parameters()) + list(model.named_buffers()) if v.device.type != "meta"}
    # ... including a quantized module's weight: its scale (and float shift) follow the dtype the module was built in, so that a
    # checkpoint saved in another float dtype does not leave bias / activations in one dtype and the weight's scale in another
    qdtype = {name: m.weight.dtype for name, m in model.named_modules() if isinstance(m, QModuleMixin) and m.weight is not None}
    loaded = model.load_state_dict(state_dict, strict=False, assign=True)
    # A checkpoint written by the reference may quantize module types this package has no counterpart for (the reference's QLayerNorm,
    # nn/qlayernorm.py): loading it silently would compute something else than what was saved - say so, loudly.
    if not_rebuilt or missing or loaded.unexpected_keys:
        import warnings

        parts = []
        if not_rebuilt:
            parts.append("no quantized counterpart for " + ", ".join(not_rebuilt[:4]) + (f" and {len(not_rebuilt) - 4} more" if len(not_rebuilt) > 4 else "")
                         + " (kept as float modules: their input / output scales are dropped)")
        if missing:
            parts.append("quantization_map names modules the model does not have: " + ", ".join(missing[:4]))
        if loaded.unexpected_keys:
            parts.append(f"{len(loaded.unexpected_keys)} state-dict entries were not used, e.g. " + ", ".join(list(loaded.unexpected_keys)[:4]))
        warnings.warn("requantize: the rebuilt model differs from the checkpoint - " + "; ".join(parts), UserWarning)
    for k, v in list(model.named_parameters()) + list(model.named_buffers()):
        if k in want and type(v.data) is torch.Tensor and v.is_floating_point() and v.dtype != want[k]:
            v.data = v.data.to(want[k])
    recast = []
    for name, m in model.named_modules():
        if name in qdtype and isinstance(m.weight, QTensor) and m.weight._scale.dtype != qdtype[name]:
            recast.append(f"{name} ({m.weight._scale.dtype} -> {qdtype[name]})")
            m.weight = torch.nn.Parameter(_cast_qweight(m.weight, qdtype[name]), requires_grad=False)
    if recast:
        import warnings

        warnings.warn("requantize: the checkpoint's scale dtype differs from the model's; scale / shift of " + ", ".join(recast[:4]) +
                      (f" and {len(recast) - 4} more" if len(recast) > 4 else "") + " were cast to the model dtype (see the docstring)", UserWarning)
    model.to(device)


def _cast_qweight(qw, dtype):
    """The same quantized weight with its float metadata (scale, float shift) in ``dtype``; integers untouched."""
    names, meta = qw.__tensor_flatten__()
    inner = {}
    for n in names:
        t = getattr(qw, n)
        inner[n] = t.to(dtype) if type(t) is torch.Tensor and t.is_floating_point() and n in ("_scale", "_shift") else t
    return type(qw).__tensor_unflatten__(inner, meta, None, None)


def freeze(model: torch.nn.Module):
    for m in model.modules():
        if isinstance(m, QModuleMixin):
            m.freeze()


def quantization_map(model: torch.nn.Module) -> Dict[str, Dict[str, str]]:
    """``{module name: {"weights": qtype name | "none", "activations": ...}}`` for every quantized module."""
    config = {}
    for name, m in model.named_modules():
        if isinstance(m, QModuleMixin):
            config[name] = {
                "weights": "none" if m.weight_qtype is None else m.weight_qtype.name,
                "activations": "none" if m.activation_qtype is None else m.activation_qtype.name,
            }
    return config


_FUSED_OUTPUT_DTYPES = (torch.int8, torch.float8_e4m3fn, torch.float8_e5m2)  # the operand pairs quanto::qbytes_mm_q serves; the activations of qbits_mm_a8_q


def _a8_gate_admits(m: QLinear) -> bool:
    """The weight formats the W4A8 / W2A8 kernel takes (csrc/qbits_a8_fused.hip, qbits_a8_supported): groups of 128 along in_features (per-channel with
    128 inputs included), a whole number of them, and out_features a multiple of 4 packed rows (8 features for int4, 16 for int2)."""
    w = m.weight
    if not (isinstance(w, WeightQBitsTensor) and _fusable(w)):
        return False
    group = w._group_size if w._group_size is not None else m.in_features
    return group == 128 and m.in_features % 128 == 0 and m.out_features % (32 // m.weight_qtype.bits) == 0


def _conv_a8_gate_admits(m: QConv2d) -> bool:
    """The layers ``quanto::qbytes_conv2d_a8_q`` serves (csrc/qconv_a8.hip): dense, zero padding given as numbers, an 8-bit weight, and a served
    (activation, weight) pair - qint8 x qint8, or qfloat8_e4m3fn / qfloat8_e5m2 activations x qfloat8_e4m3fn / qfloat8_e5m2 / qint8 weights, except
    e5m2 activations with fp16 scales (tensor/weights.py, conv2d_a8_scales_underflow)."""
    wq, aq = m.weight_qtype, m.activation_qtype
    if wq.bits != 8 or m.groups != 1 or m.padding_mode != "zeros" or isinstance(m.padding, str) or not isinstance(m.weight, WeightQBytesTensor):
        return False
    fp8 = (torch.float8_e4m3fn, torch.float8_e5m2)
    if aq.dtype == torch.int8:
        return wq.dtype == torch.int8
    if conv2d_a8_scales_underflow(aq.dtype, m.weight._scale.dtype):
        return False
    return aq.dtype in fp8 and (wq.dtype in fp8 or wq.dtype == torch.int8)


def fuse_output_quantization(model: torch.nn.Module, enable: bool = True) -> List[str]:
    """Opt in to (``enable=False``: out of) fused output quantization: every frozen ``QLinear`` with 16-bit scales and its output hook still registered is
    marked when it has an 8-bit weight qtype and an activation qtype of the same family (qint8 x qint8, qfloat8_e4m3fn x qfloat8_e4m3fn, qfloat8_e5m2 x
    qfloat8_e5m2: ``quanto::qbytes_mm_q``), or a qint4 / qint2 weight in a format the W4A8 / W2A8 kernel takes (groups of 128 or per-channel with 128
    inputs, ``in_features`` a multiple of 128, ``out_features`` a multiple of 8 / 16) and a qint8 / qfloat8_e4m3fn / qfloat8_e5m2 activation qtype
    (``quanto::qbits_mm_a8_q``); and every frozen ``QConv2d`` with bf16 / fp16 / fp32 scales and its output hook still registered when it is dense
    (``groups == 1``) with ``padding_mode == "zeros"`` and numeric padding, has an 8-bit weight qtype and a pair the quantized-activation convolution
    serves - qint8 x qint8, or qfloat8_e4m3fn / qfloat8_e5m2 activations with a qfloat8_e4m3fn / qfloat8_e5m2 / qint8 weight, but not e5m2 activations
    with fp16 scales (``quanto::qbytes_conv2d_a8_q``).  Its forward then gets the output codes from the product kernel's epilogue instead of writing
    the float output and quantizing it in a second pass - bit-identical codes, same ``output_scale``.  Also marked: every ``QLayerNorm`` with a
    qint8 / qfloat8_e4m3fn / qfloat8_e5m2 activation qtype and its output hook still registered (``quanto::layer_norm_q``: one launch reads the float
    row and stores the codes - those of the two-op sequence up to the last bits of the statistics).  Returns the names of the marked (unmarked)
    modules in ``named_modules()`` order.

    Not automatic: forward hooks registered by the user and calibration passes read a module's float output before its own hook quantizes it; a marked
    module hands them codes.  Calibrate first, then call this.  Sub-byte ``QLinear`` weights outside that format, fp32 ``QLinear`` modules, ``QConv2d``
    with sub-byte weights, groups, string or non-zero-mode padding, and other module classes are never marked; the mark is not saved with the state dict."""
    names = []
    for name, m in model.named_modules():
        if type(m) is not QLinear and type(m) is not QConv2d and type(m) is not QLayerNorm:
            continue
        if not enable:
            if m._fuse_output_quantization:
                m._fuse_output_quantization = False
                names.append(name)
            continue
        wq, aq = m.weight_qtype, m.activation_qtype
        if type(m) is QLayerNorm:  # no quantized weight, nothing to freeze
            if aq is not None and aq.dtype in _FUSED_OUTPUT_DTYPES and "output" in m._quantize_hooks:
                m._fuse_output_quantization = True
                names.append(name)
            continue
        if not (m.frozen and wq is not None and aq is not None and aq.dtype in _FUSED_OUTPUT_DTYPES and "output" in m._quantize_hooks):
            continue
        if type(m) is QConv2d:
            if m.weight._scale.dtype in (torch.bfloat16, torch.float16, torch.float32) and _conv_a8_gate_admits(m):
                m._fuse_output_quantization = True
                names.append(name)
            continue
        if m.weight._scale.dtype not in (torch.bfloat16, torch.float16):
            continue
        if (wq.bits == 8 and wq.dtype == aq.dtype) or (wq in (qint4, qint2) and _a8_gate_admits(m)):
            m._fuse_output_quantization = True
            names.append(name)
    return names
