"""Weight hand-off formats on either side of WeightAlign.

Upstream side: the reference reads its pruned dense weights from a binary ``NetParameter``
(``.caffemodel``) via ``Net::CopyTrainedLayersFrom`` (src/caffe/net.cpp) and hands each
Convolution layer's ``blobs_[0]`` to ``WeightAlign``.  protoc is not part of this image, so
``read_caffemodel`` walks the protobuf wire format directly; only the fields on this path are
decoded (field numbers from src/caffe/proto/caffe.proto):

    NetParameter      .name = 1, .layers = 2 (V1LayerParameter), .layer = 100 (LayerParameter)
    LayerParameter    .name = 1, .type = 2 (string), .blobs = 7, .convolution_param = 106
    V1LayerParameter  .name = 4, .type = 5 (enum, CONVOLUTION = 4), .blobs = 6,
                      .convolution_param = 10
    BlobProto         .num/.channels/.height/.width = 1..4, .data = 5 (packed float),
                      .shape = 7 (BlobShape.dim = 1, packed int64), .double_data = 8
    ConvolutionParameter  num_output 1, bias_term 2, pad 3, kernel_size 4, group 5, stride 6,
                      pad_h 9, pad_w 10, kernel_h 11, kernel_w 12, stride_h 13, stride_w 14,
                      dilation 18

Downstream side: ``save_aligned`` / ``load_aligned`` persist what ``WeightAlign`` produced
(the per-group CSR exactly as ``escoin_plan_get_csr`` returns it) so a deployment can skip the
dense -> CSR step and go straight to ``escoin_plan_set_csr``.

``write_caffemodel`` emits the same subset; it exists for tests and for exporting synthetic
pruned models, not as a general protobuf writer.
"""
import struct

import numpy as np

V1_CONVOLUTION = 4
V1_INNER_PRODUCT = 14
V1_DECONVOLUTION = 39
# Deconvolution layers (LayerParameter type "Deconvolution", V1LayerParameter type 39) carry the same ConvolutionParameter;
# blobs_[0] is C x num_output/group x KH x KW: its first axis is the BOTTOM's channel count (deconv_layer.cpp).
# InnerProduct layers: LayerParameter.inner_product_param = 117, V1LayerParameter.inner_product_param = 17;
# InnerProductParameter num_output 1, bias_term 2, axis 5 (default 1), transpose 6 (default false).  blobs_[0] is
# num_output x K; files written before BlobShape carry it as the legacy 1 x 1 x num_output x K.


# ---- wire format ---------------------------------------------------------------------------
def _varint(buf, pos):
    out = 0
    shift = 0
    while True:
        if pos >= len(buf):
            raise ValueError("truncated varint")
        b = buf[pos]
        pos += 1
        out |= (b & 0x7F) << shift
        if not b & 0x80:
            return out, pos
        shift += 7
        if shift > 63:
            raise ValueError("varint longer than 10 bytes")


def _fields(buf):
    """Yields (field_number, wire_type, value) for one message; value is an int (varint,
    fixed32/64 raw) or a memoryview (length-delimited)."""
    buf = memoryview(buf)
    pos = 0
    n = len(buf)
    while pos < n:
        key, pos = _varint(buf, pos)
        fno, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(buf, pos)
        elif wt == 1:
            if pos + 8 > n:
                raise ValueError("truncated fixed64")
            v = bytes(buf[pos:pos + 8])
            pos += 8
        elif wt == 2:
            ln, pos = _varint(buf, pos)
            if pos + ln > n:
                raise ValueError("truncated length-delimited field %d" % fno)
            v = buf[pos:pos + ln]
            pos += ln
        elif wt == 5:
            if pos + 4 > n:
                raise ValueError("truncated fixed32")
            v = bytes(buf[pos:pos + 4])
            pos += 4
        else:
            raise ValueError("unsupported wire type %d (field %d)" % (wt, fno))
        yield fno, wt, v


def _packed_varints(v, wt):
    if wt == 0:
        return [v]
    out = []
    pos = 0
    while pos < len(v):
        x, pos = _varint(v, pos)
        out.append(x)
    return out


def _enc_varint(x):
    x &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = x & 0x7F
        x >>= 7
        if x:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _enc_key(fno, wt):
    return _enc_varint((fno << 3) | wt)


def _enc_len(fno, payload):
    return _enc_key(fno, 2) + _enc_varint(len(payload)) + payload


def _enc_uint(fno, x):
    return _enc_key(fno, 0) + _enc_varint(int(x))


# ---- messages ------------------------------------------------------------------------------
def _parse_blob(buf):
    dims = None
    legacy = {}
    data = None
    for fno, wt, v in _fields(buf):
        if fno == 7 and wt == 2:
            dims = []
            for f2, w2, v2 in _fields(v):
                if f2 == 1:
                    dims.extend(_packed_varints(v2, w2))
        elif fno in (1, 2, 3, 4) and wt == 0:
            legacy[fno] = v
        elif fno == 5:
            if wt == 2:
                chunk = np.frombuffer(v, dtype="<f4")
            else:  # unpacked repeated float
                chunk = np.frombuffer(v, dtype="<f4", count=1)
            data = chunk if data is None else np.concatenate([data, chunk])
        elif fno == 8:
            chunk = np.frombuffer(v, dtype="<f8").astype(np.float32)
            data = chunk if data is None else np.concatenate([data, chunk])
    if data is None:
        data = np.zeros(0, np.float32)
    if dims is None:
        if legacy:
            dims = [legacy.get(i, 1) for i in (1, 2, 3, 4)]
        else:
            dims = [data.size]
    count = int(np.prod(dims)) if dims else 1
    if count != data.size:
        raise ValueError("BlobProto: shape %s holds %d values, data has %d" % (dims, count, data.size))
    return np.array(data, np.float32).reshape(dims)


def _parse_conv_param(buf):
    rep = {3: [], 4: [], 6: [], 18: []}
    one = {}
    for fno, wt, v in _fields(buf):
        if fno in rep:
            rep[fno].extend(_packed_varints(v, wt))
        elif wt == 0:
            one[fno] = v

    def hw(rep_f, h_f, w_f, default):
        if h_f in one or w_f in one:
            return one.get(h_f, default), one.get(w_f, default)
        r = rep[rep_f]
        if not r:
            return default, default
        return (r[0], r[0]) if len(r) == 1 else (r[0], r[1])

    kh, kw = hw(4, 11, 12, 0)
    ph, pw = hw(3, 9, 10, 0)
    sh, sw = hw(6, 13, 14, 1)
    d = rep[18]
    dh, dw = (1, 1) if not d else ((d[0], d[0]) if len(d) == 1 else (d[0], d[1]))
    return dict(num_output=one.get(1, 0), bias_term=bool(one.get(2, 1)), group=one.get(5, 1),
                kernel_h=kh, kernel_w=kw, pad_h=ph, pad_w=pw, stride_h=sh, stride_w=sw,
                dilation_h=dh, dilation_w=dw)


def _parse_ip_param(buf):
    one = {fno: v for fno, wt, v in _fields(buf) if wt == 0}
    axis = one.get(5, 1)
    if axis >= 1 << 31:                 # (int32 on the wire: a negative axis arrives sign-extended to 64 bits)
        axis -= 1 << 64
    return dict(num_output=one.get(1, 0), bias_term=bool(one.get(2, 1)), axis=axis, transpose=bool(one.get(6, 0)))


class CaffeLayer(object):
    """One layer of a .caffemodel: name, type string, blobs (numpy float32) and the decoded
    ConvolutionParameter (convolutions) or InnerProductParameter (inner products)."""

    def __init__(self, name, type_, blobs, conv_param=None, ip_param=None):
        self.name = name
        self.type = type_
        self.blobs = blobs
        self.conv_param = conv_param
        self.ip_param = ip_param

    @property
    def is_convolution(self):
        return self.type in ("Convolution", "ConvolutionReLU", V1_CONVOLUTION)

    @property
    def is_inner_product(self):
        return self.type in ("InnerProduct", V1_INNER_PRODUCT)

    @property
    def is_deconvolution(self):
        return self.type in ("Deconvolution", V1_DECONVOLUTION)

    def _deconv_weight(self):
        if not self.is_deconvolution or not self.blobs or not self.conv_param:
            raise ValueError("layer %s is no Deconvolution layer with blobs and a convolution_param" % self.name)
        w, p = self.blobs[0], self.conv_param
        if w.ndim != 4:
            raise ValueError("layer %s: weight blob has %d axes" % (self.name, w.ndim))
        g, m = max(int(p["group"]), 1), int(p["num_output"])
        if m % g or w.shape[0] % g or tuple(w.shape[1:]) != (m // g, p["kernel_h"], p["kernel_w"]):
            raise ValueError("layer %s: Deconvolution weight blob %s is not C x %d/%d x %d x %d" %
                             (self.name, w.shape, m, g, p["kernel_h"], p["kernel_w"]))
        return w

    def deconv_desc(self, N, H, W, relu=False):
        """The 16 ints of escoin_conv_desc for this Deconvolution layer at batch N on an H x W bottom, in ConvDesc's field
        order, for Plan(ConvDesc(*layer.deconv_desc(N, H, W)), deconv=1): C is the weight blob's first axis."""
        w, p = self._deconv_weight(), self.conv_param
        return (int(N), int(w.shape[0]), int(H), int(W), int(p["num_output"]), p["kernel_h"], p["kernel_w"], p["pad_h"], p["pad_w"],
                p["stride_h"], p["stride_w"], p["dilation_h"], p["dilation_w"], p["group"], int(len(self.blobs) > 1), int(bool(relu)))

    def _ip_weight(self):
        if not self.is_inner_product or not self.blobs:
            raise ValueError("layer %s is no InnerProduct layer with blobs" % self.name)
        w = self.blobs[0]
        if w.ndim == 4 and w.shape[:2] == (1, 1):      # the legacy 1 x 1 x M x K
            w = w.reshape(w.shape[2:])
        if w.ndim != 2:
            raise ValueError("layer %s: InnerProduct weight blob has shape %s" % (self.name, self.blobs[0].shape))
        if self.ip_param and self.ip_param["transpose"]:
            raise ValueError("layer %s: InnerProduct transpose = true is not supported" % self.name)
        if self.ip_param and self.ip_param["num_output"] not in (0, w.shape[0]):
            raise ValueError("layer %s: num_output %d, weight blob %s" % (self.name, self.ip_param["num_output"], w.shape))
        return w

    @property
    def num_output(self):
        """M of an InnerProduct layer (the weight blob's rows)."""
        return int(self._ip_weight().shape[0])

    @property
    def K(self):
        """Inputs per image of an InnerProduct layer (the weight blob's columns)."""
        return int(self._ip_weight().shape[1])

    @property
    def ip_weight(self):
        """blobs_[0] of an InnerProduct layer as num_output x K, whichever blob shape the file used."""
        return self._ip_weight()

    @property
    def ip_bias(self):
        """blobs_[1] of an InnerProduct layer as a vector, or None (bias_term = false)."""
        self._ip_weight()
        return self.blobs[1].reshape(-1) if len(self.blobs) > 1 else None

    def ip_desc(self, N, relu=False):
        """The 16 ints of escoin_conv_desc for this InnerProduct layer at batch N, in ConvDesc's field order: N images
        of K channels and one pixel, a 1x1 kernel (ConvDesc(*layer.ip_desc(N)); ConvDesc.inner_product builds the same)."""
        return (int(N), self.K, 1, 1, self.num_output, 1, 1, 0, 0, 1, 1, 1, 1, 1, int(self.ip_bias is not None), int(bool(relu)))

    def __repr__(self):
        return "CaffeLayer(%r, %r, blobs=%s)" % (self.name, self.type, [b.shape for b in self.blobs])


def _parse_layer(buf, v1):
    f_name, f_type, f_blobs, f_conv = (4, 5, 6, 10) if v1 else (1, 2, 7, 106)
    f_ip = 17 if v1 else 117
    name, type_, blobs, conv, ip = "", None, [], None, None
    for fno, wt, v in _fields(buf):
        if fno == f_name and wt == 2:
            name = bytes(v).decode("utf-8")
        elif fno == f_type:
            type_ = v if v1 else bytes(v).decode("utf-8")
        elif fno == f_blobs and wt == 2:
            blobs.append(_parse_blob(v))
        elif fno == f_conv and wt == 2:
            conv = _parse_conv_param(v)
        elif fno == f_ip and wt == 2:
            ip = _parse_ip_param(v)
    return CaffeLayer(name, type_, blobs, conv, ip)


def parse_net(buf):
    """Binary NetParameter -> (net name, [CaffeLayer])."""
    name, layers = "", []
    for fno, wt, v in _fields(buf):
        if fno == 1 and wt == 2:
            name = bytes(v).decode("utf-8")
        elif fno == 100 and wt == 2:
            layers.append(_parse_layer(v, v1=False))
        elif fno == 2 and wt == 2:
            layers.append(_parse_layer(v, v1=True))
    return name, layers


def read_caffemodel(path):
    with open(path, "rb") as f:
        return parse_net(f.read())


def conv_weights(layers):
    """{layer name: (weight M x C/g x KH x KW, bias or None)} for the convolution layers that
    carry blobs -- what Net::CopyTrainedLayersFrom would copy into blobs_[0], blobs_[1]."""
    out = {}
    for l in layers:
        if not l.is_convolution or not l.blobs:
            continue
        w = l.blobs[0]
        if w.ndim != 4:
            raise ValueError("layer %s: weight blob has %d axes" % (l.name, w.ndim))
        b = l.blobs[1].reshape(-1) if len(l.blobs) > 1 else None
        out[l.name] = (w, b)
    return out


def deconv_weights(layers):
    """{layer name: (weight C x num_output/g x KH x KW, bias or None)} for the Deconvolution layers that carry blobs; the
    weight blob is checked against the layer's ConvolutionParameter."""
    return {l.name: (l._deconv_weight(), l.blobs[1].reshape(-1) if len(l.blobs) > 1 else None)
            for l in layers if l.is_deconvolution and l.blobs}


def inner_product_weights(layers):
    """{layer name: (weight num_output x K, bias or None)} for the InnerProduct layers that carry blobs."""
    return {l.name: (l.ip_weight, l.ip_bias) for l in layers if l.is_inner_product and l.blobs}


# ---- writer (tests / synthetic exports) ------------------------------------------------------
def _enc_blob(a, legacy_dims=False):
    a = np.ascontiguousarray(a, dtype="<f4")
    out = b""
    if legacy_dims:
        dims = ([1] * (4 - a.ndim) + list(a.shape))[-4:]
        for f, d in zip((1, 2, 3, 4), dims):
            out += _enc_uint(f, d)
    else:
        out += _enc_len(7, _enc_len(1, b"".join(_enc_varint(d) for d in a.shape)))
    out += _enc_len(5, a.tobytes())
    return out


def _enc_conv_param(p):
    out = _enc_uint(1, p["num_output"]) + _enc_uint(2, int(p.get("bias_term", True)))
    out += _enc_uint(5, p.get("group", 1))
    out += _enc_uint(11, p["kernel_h"]) + _enc_uint(12, p["kernel_w"])
    out += _enc_uint(9, p.get("pad_h", 0)) + _enc_uint(10, p.get("pad_w", 0))
    out += _enc_uint(13, p.get("stride_h", 1)) + _enc_uint(14, p.get("stride_w", 1))
    dh, dw = p.get("dilation_h", 1), p.get("dilation_w", 1)
    if (dh, dw) != (1, 1):
        out += _enc_uint(18, dh) + _enc_uint(18, dw)
    return out


def _enc_ip_param(p):
    out = _enc_uint(1, p["num_output"]) + _enc_uint(2, int(p.get("bias_term", True)))
    if p.get("axis", 1) != 1:
        out += _enc_uint(5, p["axis"])
    if p.get("transpose", False):
        out += _enc_uint(6, 1)
    return out


def serialize_net(name, layers, v1=False):
    """layers: iterable of CaffeLayer.  v1=True writes the deprecated V1LayerParameter form
    (with 4-D legacy blob dims), which old pruned model zoo files still use."""
    out = _enc_len(1, name.encode("utf-8"))
    for l in layers:
        if v1:
            body = _enc_len(4, l.name.encode("utf-8"))
            body += _enc_uint(5, V1_CONVOLUTION if l.is_convolution else V1_INNER_PRODUCT if l.is_inner_product else
                              V1_DECONVOLUTION if l.is_deconvolution else 0)
            for b in l.blobs:
                body += _enc_len(6, _enc_blob(b, legacy_dims=True))
            if l.conv_param:
                body += _enc_len(10, _enc_conv_param(l.conv_param))
            if l.ip_param:
                body += _enc_len(17, _enc_ip_param(l.ip_param))
            out += _enc_len(2, body)
        else:
            body = _enc_len(1, l.name.encode("utf-8")) + _enc_len(2, str(l.type).encode("utf-8"))
            for b in l.blobs:
                body += _enc_len(7, _enc_blob(b))
            if l.conv_param:
                body += _enc_len(106, _enc_conv_param(l.conv_param))
            if l.ip_param:
                body += _enc_len(117, _enc_ip_param(l.ip_param))
            out += _enc_len(100, body)
    return out


def write_caffemodel(path, name, layers, v1=False):
    with open(path, "wb") as f:
        f.write(serialize_net(name, layers, v1=v1))


def conv_param_of(shape):
    """ConvolutionParameter dict for a synth.ConvShape."""
    return dict(num_output=shape.M, bias_term=bool(shape.bias), group=shape.group,
                kernel_h=shape.KH, kernel_w=shape.KW, pad_h=shape.pad_h, pad_w=shape.pad_w,
                stride_h=shape.stride_h, stride_w=shape.stride_w, dilation_h=shape.dil_h,
                dilation_w=shape.dil_w)


# ---- aligned (post-WeightAlign) form -----------------------------------------------------------
_ALIGNED_MAGIC = "escoin-aligned-csr-v1"


def save_aligned(path, layers):
    """layers: {name: (ConvDesc-like with the 16 int fields, (rowptr, colidx, values, nnz_per_group))}.
    Column indices are the unstretched ones (escoin_plan_get_csr(stretched=0)), so the file does not
    depend on the input geometry a later plan pads for."""
    arrays = {"magic": np.array(_ALIGNED_MAGIC), "names": np.array(sorted(layers))}
    for name, (desc, (rp, ci, va, ng)) in layers.items():
        arrays[name + "/desc"] = np.array([getattr(desc, f) for f, _ in desc._fields_], np.int32)
        arrays[name + "/rowptr"] = np.asarray(rp, np.int32)
        arrays[name + "/colidx"] = np.asarray(ci, np.int32)
        arrays[name + "/values"] = np.asarray(va, np.float32)
        arrays[name + "/nnz"] = np.asarray(ng, np.int32)
    np.savez(path, **arrays)


def load_aligned(path):
    """-> {name: (desc field list, (rowptr, colidx, values, nnz_per_group))}"""
    z = np.load(path, allow_pickle=False)
    if str(z["magic"]) != _ALIGNED_MAGIC:
        raise ValueError("%s is not an aligned-CSR file" % path)
    out = {}
    for name in z["names"].tolist():
        out[name] = (z[name + "/desc"].tolist(),
                     (z[name + "/rowptr"], z[name + "/colidx"], z[name + "/values"], z[name + "/nnz"]))
    return out


def float_bits(x):
    """Helper for tests: the IEEE-754 bits of a float32 scalar."""
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]
