"""iodine_amd: MI355X-native (gfx950) IODINE refinement step behind the reference's
``IODINE.forward / reconstruct`` module API.  Heavy imports are lazy so that
``iodine_amd.synth`` can be used without the HIP library being built."""

__all__ = ['IODINE', 'Predictive', 'Restarts', 'Adaptive', 'adaptive', 'chains', 'chain_score', 'chain_consensus', 'synth', 'parallel', 'optim', 'ari', 'checkpoint', 'data', 'engine', 'objects', 'traverse', 'matching', 'figures',
           'slot_table', 'overlap_table', 'slot_iou', 'SLOT_COLUMNS', 'components', 'clean_segmentation', 'seg_to_mask', 'Components', 'latent_kl', 'rank_dims', 'Traversal',
           'pack_gt', 'overlap', 'assign', 'match_masks', 'matched_mask_loss', 'segmentation_scores', 'SegmentationEvaluator',
           'PALETTE', 'sheet', 'layout', 'matched_colors', 'decomposition', 'trajectory_sheet', 'restarts_sheet', 'encode_png', 'write_png']


def __getattr__(name):
    if name == 'IODINE':
        from .model import IODINE
        return IODINE
    if name == 'Predictive':                                  # (what ``IODINE.predictive`` returns)
        from .model import Predictive
        return Predictive
    if name == 'Restarts':                                    # (what ``IODINE.restarts`` returns)
        from .model import Restarts
        return Restarts
    if name == 'Adaptive':                                    # (what ``IODINE.reconstruct_adaptive`` returns)
        from .adaptive import Adaptive
        return Adaptive
    if name in ('chain_score', 'chain_consensus'):
        from . import chains
        return getattr(chains, name)
    if name in ('slot_table', 'overlap_table', 'slot_iou', 'SLOT_COLUMNS', 'components', 'clean_segmentation', 'seg_to_mask', 'Components'):
        from . import objects
        return getattr(objects, name)
    if name in ('latent_kl', 'rank_dims', 'Traversal'):      # (``iodine_amd.traverse`` is the module; the function is ``traverse.traverse``)
        from . import traverse
        return getattr(traverse, name)
    if name in ('pack_gt', 'overlap', 'assign', 'match_masks', 'matched_mask_loss', 'segmentation_scores', 'SegmentationEvaluator'):
        from . import matching
        return getattr(matching, name)
    if name in ('PALETTE', 'sheet', 'layout', 'matched_colors', 'decomposition', 'trajectory_sheet', 'restarts_sheet', 'encode_png', 'write_png'):
        from . import figures
        return getattr(figures, name)
    raise AttributeError(name)
