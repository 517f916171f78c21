"""SDK clients: sync + async access to a running node's admin API.

Reference parity: infomesh/sdk/client.py (InfoMeshClient search/crawl/
suggest/status over the local HTTP API).
"""
from __future__ import annotations

from typing import Any

import httpx

DEFAULT_BASE = "http://127.0.0.1:8080"


def _search_params(query, limit, mode, include_domains, exclude_domains,
                   recency_days, facets=False,
                   facet_domains=None, top_domains=0) -> dict[str, Any]:
    """/search parameters; the domain lists go comma-separated, and only
    when given."""
    params: dict[str, Any] = {"q": query, "limit": limit, "mode": mode}
    if include_domains:
        params["include_domains"] = ",".join(include_domains)
    if exclude_domains:
        params["exclude_domains"] = ",".join(exclude_domains)
    if recency_days:
        params["recency_days"] = recency_days
    if facets:
        params["facets"] = 1
        if facet_domains:
            params["facet_domains"] = ",".join(facet_domains)
        if top_domains:
            params["top_domains"] = int(top_domains)
    return params


def _search_result(body: dict, facets: bool):
    """The hit list, as ever; for a request with facets the hits with
    the counts: {"results", "total_matches", "facets"}."""
    if not facets:
        return body["results"]
    return {"results": body["results"],
            "total_matches": body.get("total_matches"),
            "facets": body.get("facets")}


class InfoMeshClient:
    def __init__(self, base_url: str = DEFAULT_BASE, api_key: str = "",
                 timeout: float = 30.0,
                 transport: httpx.BaseTransport | None = None):
        headers = {"x-api-key": api_key} if api_key else {}
        self._client = httpx.Client(base_url=base_url, headers=headers,
                                    timeout=timeout, transport=transport)

    def search(self, query: str, limit: int = 10, mode: str = "auto",
               include_domains=None, exclude_domains=None,
               recency_days: float = 0, facets: bool = False,
               facet_domains=None, top_domains: int = 0):
        """include_domains / exclude_domains: exact domains to allow /
        block; recency_days: only documents crawled that recently.
        facets: return {"results", "total_matches", "facets"} instead of
        the hit list, with counts over every matching document;
        facet_domains: the domains to count; top_domains: how many of
        the match set's top domains to add to the facets (at most 32)."""
        r = self._client.get("/search", params=_search_params(
            query, limit, mode, include_domains, exclude_domains,
            recency_days, facets, facet_domains, top_domains))
        r.raise_for_status()
        return _search_result(r.json(), facets)

    def status(self) -> dict[str, Any]:
        r = self._client.get("/status")
        r.raise_for_status()
        return r.json()

    def index_stats(self) -> dict[str, Any]:
        r = self._client.get("/index/stats")
        r.raise_for_status()
        return r.json()

    def credits(self) -> dict[str, Any]:
        r = self._client.get("/credits/balance")
        r.raise_for_status()
        return r.json()

    def feedback(self, url: str, signal: str, query: str = "") -> bool:
        r = self._client.post("/feedback", params={
            "url": url, "signal": signal, "q": query})
        r.raise_for_status()
        return bool(r.json().get("recorded"))

    def health(self) -> bool:
        try:
            return bool(self._client.get("/health").json().get("ok"))
        except (httpx.HTTPError, ValueError):
            return False

    def close(self) -> None:
        self._client.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class AsyncInfoMeshClient:
    def __init__(self, base_url: str = DEFAULT_BASE, api_key: str = "",
                 timeout: float = 30.0,
                 transport: httpx.AsyncBaseTransport | None = None):
        headers = {"x-api-key": api_key} if api_key else {}
        self._client = httpx.AsyncClient(base_url=base_url, headers=headers,
                                         timeout=timeout,
                                         transport=transport)

    async def search(self, query: str, limit: int = 10, mode: str = "auto",
                     include_domains=None, exclude_domains=None,
                     recency_days: float = 0, facets: bool = False,
                     facet_domains=None, top_domains: int = 0):
        """As InfoMeshClient.search."""
        r = await self._client.get("/search", params=_search_params(
            query, limit, mode, include_domains, exclude_domains,
            recency_days, facets, facet_domains, top_domains))
        r.raise_for_status()
        return _search_result(r.json(), facets)

    async def status(self) -> dict[str, Any]:
        r = await self._client.get("/status")
        r.raise_for_status()
        return r.json()

    async def close(self) -> None:
        await self._client.aclose()

    async def __aenter__(self):
        return self

    async def __aexit__(self, *exc):
        await self.close()
        return False
