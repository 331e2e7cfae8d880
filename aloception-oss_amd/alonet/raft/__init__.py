from .corr import AlternateCorrBlock, CorrBlock, TrainableAlternateCorrBlock
from .criterion import RAFTCriterion
from .raft import RAFT, RAFTBase
from .raft_small import RAFTSmall

__all__ = ["AlternateCorrBlock", "CorrBlock", "RAFT", "RAFTBase", "RAFTCriterion", "RAFTSmall", "TrainableAlternateCorrBlock"]
