"""The layer graph a parsed prototxt describes, in a comparable form, and one digest per layer of it.

tests/golden/reference_graphs.json holds the digests of the reference's own net definitions (written by
tests/golden/make_reference_graphs.py); tests/test_proto_netspec.py holds the builders of fcn_object_detector_amd.models to them."""
import hashlib
import json

from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec


def signature(msg, phase):
    spec = NetSpec(msg, phase)
    out = []
    for l in spec.layers:
        d = [l.type, l.name, tuple(l.bottoms), tuple(l.tops), tuple(l.lr_mult), tuple(l.decay_mult), tuple(l.loss_weight)]
        for key in ("convolution_param", "pooling_param", "lrn_param", "power_param", "dropout_param", "eltwise_param"):
            p = l.msg.get(key)
            if p is None:
                continue
            items = []
            for k, v in sorted(p.fields.items()):
                vals = []
                for x in v:
                    if isinstance(x, proto.Msg):
                        vals.append(tuple((kk, tuple(vv)) for kk, vv in sorted(x.fields.items()) if kk != "std"))
                    else:
                        vals.append(float(x) if isinstance(x, (int, float)) and not isinstance(x, bool) else x)
                items.append((k, tuple(vals)))
            d.append((key, tuple(items)))
        out.append(tuple(d))
    return spec.input_shapes, out


def _canonical(x):
    if isinstance(x, (tuple, list)):
        return [_canonical(v) for v in x]
    return float(x) if isinstance(x, (int, float)) and not isinstance(x, bool) else x      # 0 and 0.0 are the same value


def layer_digests(layers):
    """One digest per layer of signature()'s second value: equal digests <=> equal layers (type, name, bottoms, tops,
    multipliers, loss weights and every parameter of the six parameter messages signature() reads)."""
    return [hashlib.sha256(json.dumps(_canonical(l)).encode()).hexdigest()[:16] for l in layers]
