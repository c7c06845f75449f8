"""Argument groups PEGASUS re-uses by appending to sys.argv (pegasus.py:152-154): only the fields the render
path reads are kept (sh_degree, source/model paths, white_background, data_device; the three pipeline flags), and the
3DGS optimisation fields pegasus_amd.train.training reads."""
from argparse import ArgumentParser, Namespace


class GroupParams:
    pass


class ParamGroup:
    def __init__(self, parser: ArgumentParser, name: str, fill_none=False):
        group = parser.add_argument_group(name)
        for key, value in vars(self).items():
            shorthand = key.startswith("_")
            key = key[1:] if shorthand else key
            t = type(value)
            value = value if not fill_none else None
            flags = ["--" + key] + (["-" + key[0:1]] if shorthand else [])
            if t == bool:
                group.add_argument(*flags, default=value, action="store_true")
            else:
                group.add_argument(*flags, default=value, type=t)

    def extract(self, args):
        group = GroupParams()
        for k, v in vars(args).items():
            if k in vars(self) or ("_" + k) in vars(self):
                setattr(group, k, v)
        return group


class ModelParams(ParamGroup):
    def __init__(self, parser, sentinel=False):
        self.sh_degree = 3
        self._source_path = ""
        self._model_path = ""
        self._images = "images"
        self._resolution = -1
        self._white_background = False
        self.data_device = "cuda"
        self.eval = False
        self.masks = ""                # per-image object masks: a directory, "alpha" or "" (pegasus_amd.train.MASK_DEFAULTS)
        super().__init__(parser, "Loading Parameters", sentinel)


class PipelineParams(ParamGroup):
    def __init__(self, parser):
        self.convert_SHs_python = False
        self.compute_cov3D_python = False
        self.debug = False
        super().__init__(parser, "Pipeline Parameters")


class OptimizationParams(ParamGroup):
    def __init__(self, parser):
        self.iterations = 30_000
        # the 3DGS optimisation fields with their usual defaults (pegasus_amd.train.OPTIMIZATION_DEFAULTS)
        self.position_lr_init = 0.00016
        self.position_lr_final = 0.0000016
        self.position_lr_delay_mult = 0.01
        self.position_lr_max_steps = 30_000
        self.feature_lr = 0.0025
        self.opacity_lr = 0.05
        self.scaling_lr = 0.005
        self.rotation_lr = 0.001
        self.percent_dense = 0.01
        self.lambda_dssim = 0.2
        self.densification_interval = 100
        self.opacity_reset_interval = 3000
        self.densify_from_iter = 500
        self.densify_until_iter = 15_000
        self.densify_grad_threshold = 0.0002
        self.random_background = False
        self.lambda_alpha = 0.5        # weight of mean|alpha - mask| when training from masks
        super().__init__(parser, "Optimization Parameters")


def get_combined_args(parser: ArgumentParser):
    import sys
    return parser.parse_args(sys.argv[1:])
