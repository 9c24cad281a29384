// aesw_entry.h -- what an entry point of a library next to libaesw.so says before it launches: the preamble (a group context
// is refused, a null one is an invalid argument), the one refusal that leaves its reason in last_error, and -- through
// aesw_entry_rules.h, which needs neither ROCm nor the context -- the argument rules the libraries share.  Host code.
#pragma once
#include <string>

#include "aesw_ctx.h"
#include "aesw_entry_rules.h"

namespace aesw {

// if (int rc = entry_refused(ctx, call)) return rc;
inline int entry_refused(aesw_ctx *ctx, const char *call) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, call);
    return ctx ? AESW_OK : AESW_ERR_INVALID_ARG;
}
static_assert(AESW_OK == 0, "a refusal is a status that is not 0");

inline int refuse(aesw_ctx *ctx, const char *call, const char *why, int status = AESW_ERR_INVALID_ARG) {
    if (ctx) ctx->last_error = std::string(call) + ": " + why;
    return status;
}

}  // namespace aesw
