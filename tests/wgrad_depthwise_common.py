"""Shared by test_wgrad_depthwise_host.py and test_wgrad_depthwise_gpu.py: the cases of plan option "wgrad_depthwise" with what
align_rules.h dww_plan gives them on 256 CUs -- the lane's pixel count px (the kernel instantiation) and the slices of a full batch.
The host test pins both on the rule; the GPU test asserts the slices on the stat."""
import depthwise_common as dc

OPTS = ((0, 0), (1, 1), (2, 3))         # ("depthwise_band_rows", "wgrad_depthwise_slices")
# depthwise_common's shapes: so few units that the rule's band is 1 row and px 1 whatever "depthwise_band_rows" says; their (image,
# band) pairs.  (On few CUs the band stays taller: (2, 3) on 3x3_s1 then gives 10 pairs in slices of 4, 4 and 2 -- the host test's.)
PAIRS = dict(zip(dc.SHAPES, (18, 12, 16, 12, 18, 21, 5, 6, 16)))
# 3x3, pad 1, unpruned shapes that reach the other instantiations, as name: ((N, C = M = group, H, W), px, slices under S = 3):
NEW = {"bands2": ((2, 700, 8, 8), 1, 3),        # bands of 2 rows: items of two output rows, 8 pairs in slices of 3, 3 and 2 across the images
       "w256": ((1, 2, 5, 256), 4, 3),          # px 4, a row = 64 runs: 16-byte loads of top_diff, the pass without the select
       "w254": ((1, 2, 5, 254), 4, 3),          # px 4, OW no multiple of 4: scalar loads, a last run of 2 live pixels
       "w128": ((1, 2, 5, 128), 2, 3),          # px 2, 8-byte loads, the pass without the select
       "w130": ((1, 2, 5, 130), 2, 3),          # px 2, 65 runs: 8-byte loads with dead lanes in the second item
       "w129": ((1, 2, 5, 129), 2, 3),          # px 2, odd OW: scalar loads, a last run of 1 live pixel
       "c1024": ((1, 1024, 32, 32), 4, 2)}      # px 4 and bands of 8 rows: 4 pairs in slices of 2
# (name, fuse_relu, options, px, slices)
CASES = [(n, relu, o, 1, (PAIRS[n], 1, 3)[i]) for relu, names in ((False, dc.SHAPES), (True, ("3x3_s1", "3x3_s2", "mult2")))
         for n in names for i, o in enumerate(OPTS)] + [(n, relu, (0, 3), px, sl) for n, (_, px, sl) in NEW.items() for relu in (False, True)]
_NEW = {}


def case(synth, name):
    """(shape, weights, bottom, bias, top_diff), made once per name."""
    if name not in NEW:
        return dc.case(synth, name)
    if name not in _NEW:
        N, C, H, W = NEW[name][0]
        s = synth.shape(name, N, C, H, W, C, 3, pad=1, group=C, sparsity=0.0)
        _NEW[name] = (s, synth.pruned_weights(s, 11), synth.activations(s, 12), synth.bias_vector(s, 13),
                      synth.uniform(21, N * C * H * W).reshape(N, C, H, W))
    return _NEW[name]
