wtp_internal.h	s#constexpr bool RES_EARLY_POLL_STORES = true;#constexpr bool RES_EARLY_POLL_STORES = false;#
