// Kernel instantiations for the 500-job node bucket (one TU per bucket so the
// instantiations compile in parallel).
#include "pfsp_engine.hpp"

namespace tts {
TTS_PFSP_DEFINE_BUCKET(500)
// 201-500 jobs on front nodes with 512-bit job sets (TTS_FRONT_WIDE=2)
TTS_PFSP_DEFINE_FRONT_BUCKET(500)
}  // namespace tts
