"""A stand-in for upstream's DepthDecoder, made of this project's mirror classes under upstream's attribute names, for the tests of
adopt_depth_front: `feature_extractor` (conv1, bn1, relu, maxpool, layer), `cost_volume_builder`, `resnet_layer_2..4`, `expansion5..1`,
`disp4..1`, `height`, `width`, `channels`, `use_input_image_in_skip_connection`.  Its own forward is the UNADOPTED one the tests compare
with: the extractor's modules called one by one on the target and then on the sources, the cost volume, the three strided layers, the
expansion layers with their skips and the heads.
"""
import torch
from torch import nn

from macarons_amd.networks import ManyDepth


def resnet_front(Cin=3, C=64, n_blocks=2, bias=False):
    """What upstream's FeatureExtractor is constructed from: anything with conv1, bn1, relu, maxpool and layer1."""
    net = nn.Module()
    net.conv1 = nn.Conv2d(Cin, C, kernel_size=7, stride=2, padding=3, bias=bias)
    net.bn1, net.relu, net.maxpool = nn.BatchNorm2d(C), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    net.layer1 = nn.Sequential(*[ManyDepth.BasicBlock(C, C) for _ in range(n_blocks)])
    return net


def randomize_batch_norms(module, seed):
    """Running statistics and affine parameters away from their initial 0 / 1, so that an eval-mode BatchNorm is no identity."""
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)
    return module


def strided_layer(Cin, Cout):
    down = nn.Sequential(nn.Conv2d(Cin, Cout, kernel_size=1, stride=2, bias=False), nn.BatchNorm2d(Cout))
    return nn.Sequential(ManyDepth.BasicBlock(Cin, Cout, stride=2, downsample=down), ManyDepth.BasicBlock(Cout, Cout))


class MeanBuilder(nn.Module):
    """A cost-volume builder for the CPU (the mirror's sweep exists on HIP only): the same call, relu(conv_reduce(cat(x, mean of the
    sources' features)))."""

    def __init__(self, C):
        super().__init__()
        self.conv_reduce = nn.Conv2d(2 * C, C, 3, padding=1)

    def forward(self, x, R, T, zfar, x_alpha, R_alpha, T_alpha, zfar_alpha, device=None):
        return torch.relu(self.conv_reduce(torch.cat((x, x_alpha.mean(1)), 1)))


class StandInDecoder(nn.Module):
    def __init__(self, H=32, W=64, n_alpha=2, builder=None):
        super().__init__()
        self.height, self.width, self.channels, self.use_input_image_in_skip_connection = H, W, 3, True
        self.feature_extractor = ManyDepth.FeatureExtractor(resnet_front())
        self.cost_volume_builder = builder if builder is not None else ManyDepth.CostVolumeBuilder(
            height=H, width=W, feature_height=H // 4, feature_width=W // 4, feature_channels=64, n_alpha=n_alpha, d_min=0.5, d_max=20.0,
            n_depth=8, output_channels=64)
        self.resnet_layer_2, self.resnet_layer_3, self.resnet_layer_4 = strided_layer(64, 128), strided_layer(128, 256), strided_layer(256, 512)
        size = lambda k: (H // k, W // k + (W % k > 0))                                                   # noqa: E731
        self.expansion5 = ManyDepth.ExpansionLayer(512, 256, 256, size(16), additional_channels=256)
        self.expansion4 = ManyDepth.ExpansionLayer(256, 128, 128, size(8), additional_channels=128)
        self.expansion3 = ManyDepth.ExpansionLayer(128, 64, 64, size(4), additional_channels=64)
        self.expansion2 = ManyDepth.ExpansionLayer(64, 32, 32, size(2), additional_channels=64)
        self.expansion1 = ManyDepth.ExpansionLayer(32, 16, 16, (H, W), additional_channels=3)
        self.disp4, self.disp3, self.disp2, self.disp1 = (ManyDepth.DisparityLayer(c) for c in (128, 64, 32, 16))
        randomize_batch_norms(self, 5)

    def forward(self, x, R, T, zfar, x_alpha, R_alpha, T_alpha, zfar_alpha, device):
        fe = self.feature_extractor
        B, A = x.shape[0], x_alpha.shape[1]
        conv1 = fe.relu(fe.bn1(fe.conv1(x)))
        layer1 = fe.layer(fe.maxpool(conv1))
        a = fe.relu(fe.bn1(fe.conv1(x_alpha.reshape(-1, self.channels, self.height, self.width))))
        layer1_alpha = fe.layer(fe.maxpool(a)).view(B, A, 64, self.height // 4, self.width // 4)
        layer2 = self.resnet_layer_2(self.cost_volume_builder(layer1, R, T, zfar, layer1_alpha, R_alpha, T_alpha, zfar_alpha, device=device))
        layer3 = self.resnet_layer_3(layer2)
        i5 = self.expansion5(x=self.resnet_layer_4(layer3), x_add=layer3)
        i4 = self.expansion4(x=i5, x_add=layer2)
        i3 = self.expansion3(x=i4, x_add=layer1)
        i2 = self.expansion2(x=i3, x_add=conv1)
        i1 = self.expansion1(x=i2, x_add=x)
        return self.disp1(i1), self.disp2(i2), self.disp3(i3), self.disp4(i4)


def decoder_inputs(B, A, H, W, seed=3):
    """(x, R, T, zfar, x_alpha, R_alpha, T_alpha, zfar_alpha): images in (0,1), the target at the origin, the sources shifted sideways."""
    g = torch.Generator().manual_seed(seed)
    x, x_alpha = torch.rand(B, 3, H, W, generator=g), torch.rand(B, A, 3, H, W, generator=g)
    R, T = torch.eye(3).expand(B, 3, 3).contiguous(), torch.zeros(B, 3)
    R_alpha = torch.eye(3).expand(B, A, 3, 3).contiguous()
    T_alpha = torch.stack([torch.tensor([0.1 * (a + 1), 0.0, 0.0]) for a in range(A)]).expand(B, A, 3).contiguous()
    return x, R, T, 20.0, x_alpha, R_alpha, T_alpha, 20.0
