"""The comparand of the bf16 VGG16 path: the oracle's Keras graphs under the storage model the product's bf16 VGG16 uses.

``oracle.keras_ref.KerasGraphs(mixed=True)`` rounds the ResNet blocks and rpn_conv1 only (its ``_bf16_layer``), so it does not
describe a bf16 VGG16.  This subclass does, with nothing but what the oracle exports (``conv2d``, ``pool2d``, ``roi_resize`` and its
quantisers ``q`` / ``qw``):

* ``_bf16_layer`` also names ``block*_conv*``, ``fc1`` and ``fc2`` (their filters are rounded once, ``qw``);
* ``vgg_base`` rounds the pixels once and every convolution's ReLU output once (``q``); a max-pool rounds nothing;
* ``vgg_classifier`` rounds the RoI crops, the fc1 / fc2 filters and their ReLU outputs; the two dense layers are in full precision.

With ``mixed=False`` every quantiser is the identity and the two overrides reproduce ``KerasGraphs.vgg_base`` / ``vgg_classifier``
exactly (tests/test_vgg_bf16_cpu.py)."""
import numpy as np
import torch

from oracle.keras_ref import KerasGraphs, _t, pool2d, roi_resize


class VggBf16Graphs(KerasGraphs):
    @staticmethod
    def _bf16_layer(name):
        return KerasGraphs._bf16_layer(name) or (name.startswith("block") and "_conv" in name) or name in ("fc1", "fc2")

    def vgg_base(self, x):
        x = self.q(_t(x, self.dtype))
        for blk, n in ((1, 2), (2, 2), (3, 3), (4, 3), (5, 3)):
            for i in range(1, n + 1):
                x = self.q(self.conv(x, "block%d_conv%d" % (blk, i), padding="same").clamp(min=0))
            if blk < 5:
                x = pool2d(x, 2, 2, True)
        return x

    def _fc(self, x, name):
        k, b = (_t(t, x.dtype) for t in self.w[name])
        if self.mixed and self._bf16_layer(name):
            k = self.qw(k)
        return self.q((x @ k + b).clamp(min=0))

    def vgg_classifier(self, feat, rois, num_classes):
        crops = roi_resize(np.asarray(feat[0].to(torch.float32)), np.asarray(rois), 7)
        x = self.q(torch.as_tensor(crops).to(self.dtype)).reshape(len(crops), -1)
        x = self._fc(self._fc(x, "fc1"), "fc2")
        cls = torch.softmax(self._dense(x, "dense_class_%d" % num_classes), dim=1)
        reg = self._dense(x, "dense_reg_%d" % num_classes)
        return cls, reg
