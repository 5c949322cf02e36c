"""viterbidecodercpp_amd -- MI355X (gfx950) implementation of the Viterbi update()+chainback() hot path.

Product code: csrc/ (HIP kernels + C ABI, built to libvit_hip.so) and the host-side mirror of the reference's decoder
interface in decoder.py -- the outer chain behind the decoder (marker search, frame extraction, Reed-Solomon, de-interleaver,
derandomiser, frame check) in outer.py, the tensor rules of both in _args.py --, with the chunked stream receivers in stream.py the LTE rate matching in front of the tail-biting decode in lte.py and the DAB profiles, interleaver and dispersal in dab.py, the DAB+ superframes behind them in dabplus.py, the 802.11a/g OFDM data path in wifi.py, the DVB-T inner de-interleaver and its receiver in dvbt.py, the IS-95A forward traffic channel (de-interleave, combine, blind rate decision) in is95.py, GSM channel decoding (burst de-interleavers, Fire code, TCH/FS frames, two receivers) in gsm.py.  codes.py / synth.py hold constants and synthetic-input generation for the measurement.
"""
from .codes import COMMON_CODES, Code, DecoderConfig, get_decoding_config, SOFT16, SOFT8, HARD8  # noqa: F401
from .decoder import (BatchDecoder, DecodePipeline, ViterbiBranchTable, ViterbiDecoder_Config, ViterbiDecoder_Core,  # noqa: F401
                      ViterbiDecoder_HIP, pack_blob)
from .stream import MultiStreamDecoder, StreamDecoder  # noqa: F401
from .sync import enumerate_hypotheses  # noqa: F401
from .frame_sync import CCSDS_ASM, DVB_SYNC, ccsds_randomizer, frames_extract_numpy, marker_lock_numpy, marker_search_numpy  # noqa: F401
from .reed_solomon import (CCSDS_RS_255_223, CCSDS_RS_255_223_DUAL, CCSDS_RS_255_239, CCSDS_RS_255_239_DUAL, DVB_RS_204_188, RSCode,  # noqa: F401
                           rs_decode_numpy, rs_encode_numpy)
from .dvb import (DVB_INTERLEAVER, conv_deinterleave_numpy, conv_interleave_numpy, dvb_derandomize_numpy, dvb_prbs,  # noqa: F401
                  dvb_randomize_numpy)
from .crc import (CCSDS_CRC16, DAB_CRC16, LTE_CRC8, LTE_CRC16, LTE_CRC24A, LTE_CRC24B, MPEG2_CRC32, STOCK_CRC_CODES, WIFI_FCS, CRCCode,  # noqa: F401
                  crc_append_numpy, crc_field_numpy, crc_numpy)
from .lte import (LTE_CC_COLUMN_PERMUTATION, lte_gold_sequence, lte_rate_dematch_numpy, lte_rate_match_map, lte_rate_match_numpy,  # noqa: F401
                  pdcch_candidates)
from .dab import (FIC_PROFILE, PI_X, DabProfile, DabSubchannelDecoder, dab_depuncture_numpy, dab_energy_dispersal_numpy, dab_prbs,  # noqa: F401
                  dab_puncture_numpy, dab_time_deinterleave_numpy, dab_time_interleave_numpy, eep_profile, puncture_vector)
from .dabplus import (DABPLUS_RS_120_110, FIRECODE, DabPlusDecoder, dabplus_au_table_numpy, dabplus_lock_numpy,  # noqa: F401
                      dabplus_superframe_numpy, dabplus_sync_numpy, firecode_hit_numpy)
from .wifi import (WIFI_POLYNOMIALS, WIFI_RATES, WifiDecoder, WifiRate, wifi_deinterleave_numpy, wifi_descramble_numpy,  # noqa: F401
                   wifi_interleave_map, wifi_ppdu_numpy, wifi_scrambler_numpy, wifi_signal_field_numpy, wifi_signal_parse_numpy)
from .dvbt import (DVBT_MODES, DVBT_RATES, DvbtDecoder, DvbtMode, dvbt_deinterleave_numpy, dvbt_interleave_numpy, dvbt_puncture_numpy,  # noqa: F401
                   dvbt_steps_per_symbol, dvbt_symbol_permutation)
from .is95 import (IS95_CRC8, IS95_CRC12, IS95_POLYNOMIALS, IS95_RATE_SET_1, Is95Rate, Is95TrafficDecoder, is95_deinterleave_numpy,  # noqa: F401
                   is95_permutation, is95_rate_decide_numpy, is95_traffic_frame_numpy)
from .gsm import (GSM_BLOCK, GSM_DIAGONAL, GSM_POLYNOMIALS, GSM_RACH_CRC6, GSM_SCH_CRC10, GSM_TCHFS_CRC3, GsmControlDecoder, GsmTchfDecoder,  # noqa: F401
                  gsm_deinterleave_numpy, gsm_facch_steal_numpy, gsm_fire_encode_numpy, gsm_fire_numpy, gsm_interleave_map, gsm_tchfs_bursts_numpy,
                  gsm_tchfs_class1_numpy, gsm_tchfs_numpy, gsm_xcch_bursts_numpy)
from . import _lib, crc, dab, dabplus, dist, dvb, dvbt, frame_sync, gsm, is95, lte, reed_solomon, sync, synth, wifi  # noqa: F401

__all__ = ["GSM_BLOCK", "GSM_DIAGONAL", "GSM_POLYNOMIALS", "GSM_RACH_CRC6", "GSM_SCH_CRC10", "GSM_TCHFS_CRC3", "GsmControlDecoder", "GsmTchfDecoder",
           "gsm_deinterleave_numpy", "gsm_facch_steal_numpy", "gsm_fire_encode_numpy", "gsm_fire_numpy", "gsm_interleave_map", "gsm_tchfs_bursts_numpy",
           "gsm_tchfs_class1_numpy", "gsm_tchfs_numpy", "gsm_xcch_bursts_numpy", "IS95_CRC8", "IS95_CRC12", "IS95_POLYNOMIALS", "IS95_RATE_SET_1", "Is95Rate", "Is95TrafficDecoder", "is95_deinterleave_numpy", "is95_permutation",
           "is95_rate_decide_numpy", "is95_traffic_frame_numpy", "DVBT_MODES", "DVBT_RATES", "DvbtDecoder", "DvbtMode", "dvbt_deinterleave_numpy", "dvbt_interleave_numpy", "dvbt_puncture_numpy",
           "dvbt_steps_per_symbol", "dvbt_symbol_permutation", "WIFI_POLYNOMIALS", "WIFI_RATES", "WifiDecoder", "WifiRate", "wifi_deinterleave_numpy", "wifi_descramble_numpy", "wifi_interleave_map",
           "wifi_ppdu_numpy", "wifi_scrambler_numpy", "wifi_signal_field_numpy", "wifi_signal_parse_numpy", "WIFI_FCS", "DABPLUS_RS_120_110", "FIRECODE", "DabPlusDecoder", "dabplus_au_table_numpy", "dabplus_lock_numpy", "dabplus_superframe_numpy",
           "dabplus_sync_numpy", "firecode_hit_numpy", "FIC_PROFILE", "PI_X", "DabProfile", "DabSubchannelDecoder", "dab_depuncture_numpy", "dab_energy_dispersal_numpy", "dab_prbs", "dab_puncture_numpy",
           "dab_time_deinterleave_numpy", "dab_time_interleave_numpy", "eep_profile", "puncture_vector", "LTE_CC_COLUMN_PERMUTATION", "lte_gold_sequence", "lte_rate_dematch_numpy", "lte_rate_match_map", "lte_rate_match_numpy", "pdcch_candidates",
"CCSDS_CRC16", "DAB_CRC16", "LTE_CRC8", "LTE_CRC16", "LTE_CRC24A", "LTE_CRC24B", "MPEG2_CRC32", "STOCK_CRC_CODES", "CRCCode",
           "crc_append_numpy", "crc_field_numpy", "crc_numpy", "DVB_INTERLEAVER", "conv_deinterleave_numpy", "conv_interleave_numpy", "dvb_derandomize_numpy", "dvb_prbs", "dvb_randomize_numpy",
           "CCSDS_RS_255_223", "CCSDS_RS_255_223_DUAL", "CCSDS_RS_255_239", "CCSDS_RS_255_239_DUAL", "DVB_RS_204_188", "RSCode",
           "rs_decode_numpy", "rs_encode_numpy", "CCSDS_ASM", "DVB_SYNC", "ccsds_randomizer", "frames_extract_numpy", "marker_lock_numpy", "marker_search_numpy", "COMMON_CODES", "Code", "DecoderConfig", "get_decoding_config", "SOFT16", "SOFT8", "HARD8", "BatchDecoder", "DecodePipeline",
           "MultiStreamDecoder", "StreamDecoder", "ViterbiBranchTable", "ViterbiDecoder_Config", "ViterbiDecoder_Core", "ViterbiDecoder_HIP", "enumerate_hypotheses", "pack_blob"]
